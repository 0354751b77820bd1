/*
 * cream_amd.h — C ABI of libcream_amd.so (MI355X / gfx950 hot path of microsoft/Cream).
 *
 * Every entry point is `extern "C"`, takes plain device/host pointers, sizes and a
 * `hipStream_t` passed as `void*`, returns 0 on success or a negative CREAM_ERR_* code,
 * never throws, never synchronises, never allocates device memory.  No torch types.
 *
 * Each declaration cites the reference interface (file:line under the reference
 * checkout) that it replaces.  INTEGRATION.md shows the binding a maintainer of the
 * reference would add on top of this header.
 */
#ifndef CREAM_AMD_H_
#define CREAM_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes ---------------------------------------------------------------- */
#define CREAM_OK               0
#define CREAM_ERR_BAD_ARG     -1  /* null pointer, negative size, unsupported stride    */
#define CREAM_ERR_BAD_DTYPE   -2  /* dtype enum not supported by this entry point        */
#define CREAM_ERR_LAUNCH      -3  /* hipLaunchKernel reported an error (see hipGetLastError) */
#define CREAM_ERR_TOO_LARGE   -4  /* shape exceeds what the kernel family supports       */
/* the finer codes of the cream_evit_* checks (the older entry points fold them into BAD_ARG) */
#define CREAM_ERR_CHANNEL_STRIDE -5  /* the channel stride of a (B, H, W, C) view is not 1      */
#define CREAM_ERR_BAD_STRIDE  -6  /* a batch / row / column stride is negative, not a multiple of 8, or tokens overlap */
#define CREAM_ERR_BAD_SHAPE   -7  /* a channel count or a map size outside the covered range */

/* ---- element types (the "dtype" argument) ------------------------------------------ */
#define CREAM_F32   0
#define CREAM_F16   1
#define CREAM_BF16  2   /* not in the reference (AT_DISPATCH_FLOATING_TYPES_AND_HALF only) */
#define CREAM_F64   3

/* Version handshake.  Replaces `version()` of the pybind module `rpe_index_cpp`
 * (iRPE/DeiT-with-iRPE/rpe_ops/rpe_index.cpp:126-128; asserted == "1.2.0" at
 * rpe_ops/rpe_index.py:5-8).  Returns a static string. */
const char* cream_version(void);

/* Build tag of this library ("gfx950;hipcc ...") for logs. */
const char* cream_build_info(void);

/* ---- rpe_index: bucketed relative-position gather / scatter ----------------------- */

/* Y[b,h,i,j] = in[b,h,i, idx[i,j]]          (device pointers)
 * Replaces rpe_index_forward_gpu + rpe_index_forward_gpu_kernel
 * (iRPE/DeiT-with-iRPE/rpe_ops/rpe_index_cuda.cu:24-40,54-94).
 *   y    : (B,H,Lq,Lk) contiguous, caller-allocated
 *   in   : (B,H,Lq,nb) with ELEMENT strides s0..s3 (the reference passes
 *          input.strides(), rpe_index_cuda.cu:76,91 — iRPE hands over a transposed
 *          view, irpe.py:639-642)
 *   idx  : (Lq,Lk) contiguous int32 in [0,nb)  (not range-checked, as in the reference)
 * Pure data movement: results are bit-exact for every dtype. */
int cream_rpe_index_fwd(void* y, const void* in, const int32_t* idx,
                        int B, int H, int Lq, int Lk, int nb,
                        int64_t s0, int64_t s1, int64_t s2, int64_t s3,
                        int dtype, void* stream);

/* gin[b,h,i,u] (+)= sum_{j : idx[i,j]==u} gout[b,h,i,j]     (device pointers)
 * Replaces rpe_index_backward_gpu + rpe_index_backward_gpu_kernel
 * (rpe_index_cuda.cu:42-52,96-140).  accumulate != 0: `gin` is updated in place exactly
 * like the reference (whose caller zero-fills it, rpe_ops/rpe_index.py:51);
 * accumulate == 0: `gin` is overwritten and need not be initialised (saves the memset
 * and one read of gin).  All three tensors contiguous.  Unlike the reference's global atomics the summation order is FIXED:
 * gin_initial + g[j=0] + g[j=1] + ... in ascending j — bit-reproducible, and
 * bit-identical to a sequential CPU loop for f32/f64.  f16/bf16 accumulate in f32
 * and round once. */
int cream_rpe_index_bwd(void* gin, const void* gout, const int32_t* idx,
                        int B, int H, int Lq, int Lk, int nb,
                        int dtype, int accumulate, void* stream);

/* Host (CPU-tensor) entry points — the reference module also exports forward_cpu /
 * backward_cpu (rpe_index.cpp:8-73, 82-124) and BASELINE config 1 runs on them.
 * These are a separate implementation for HOST pointers, multi-threaded with
 * std::thread over (b,h,i) rows; they are never used for device tensors.
 * Same contracts as above (host fwd requires contiguous `in`, like the reference's
 * input.contiguous() at rpe_index.cpp:28). */
int cream_rpe_index_fwd_host(void* y, const void* in, const int32_t* idx,
                             int B, int H, int Lq, int Lk, int nb, int dtype);
int cream_rpe_index_bwd_host(void* gin, const void* gout, const int32_t* idx,
                             int B, int H, int Lq, int Lk, int nb, int dtype);

/* ---- fused attention with AutoFormer's 2-D relative position bias -------------------- */

/* Padded token count used by the side buffers below: N rounded up to a multiple of 32. */
int cream_attn_rpe2d_padded_len(int N);

/* Number of partial table-gradient blocks cream_attn_rpe2d_bwd writes for a (B, H) problem on the current device:
 * one per persistent workgroup of its dK/dV kernel, min(B*H, compute units). */
int cream_attn_rpe2d_dtab_parts(int B, int H);

/* Which backward runs for the AutoFormer geometry (N = 197, 14 x 14 grid, max_relative_position 14) in bf16:
 * 0 = the two-launch backward (csrc/attn_rpe2d_bwd.hpp); 1 = the one-pass kernel (csrc/attn_rpe2d_bwd1.hpp: K, V, Q, dO of one (b, h) whole in LDS, P / dS
 * exchanged between the query-tile and key-tile owners through LDS; the side buffers dlt / qe / de / delta are not used as
 * such — the first 32 KB of dlt carry the bf16 operand images of the tables); 2 = the same pass with the two roles on separate
 * waves (csrc/attn_rpe2d_bwd2.hpp: 7 query-tile owners + 5 waves sharing the 14 key-side jobs, the table gradients accumulated in
 * registers over all items of a workgroup and written once) — the DEFAULT.  dq / dk / dv of modes 1 and 2 are bit-identical; the
 * per-workgroup table-gradient partials of mode 2 are the sums mode 0 forms (one fp32 chain per workgroup).  onepass < 0 only
 * queries.  Returns the previous setting; the initial one comes from CREAM_ATTN_BWD1 in the environment (default 2).
 * (What autograd derives for multihead_super.py:135-154 in every mode; a switch for same-box A/B measurements.) */
int cream_attn_rpe2d_bwd_mode(int onepass);

/* The attention core of AttentionSuper.forward between the qkv and proj GEMMs
 * (AutoFormer/model/module/multihead_super.py:135-154) with the relative position
 * embeddings of RelativePosition2D_super.forward (multihead_super.py:40-66) folded in:
 *     A[i,j] = scale * ( q_i.k_j + q_i.(Tkv[iv[i,j]] + Tkh[ih[i,j]]) )
 *     P = softmax_j(A)          (attention dropout 0 — the supernet recipe's value; cream_attn_rpe2d_fwd_drop below takes p > 0)
 *     O_i = sum_j P[i,j] * ( v_j + Tvv[iv[i,j]] + Tvh[ih[i,j]] )
 * for every (b, h); head_dim is 64 (supernet_transformer.py:243).  iv/ih are the
 * reference's index matrices for a gh x gw token grid behind one class token
 * (N = gh*gw + 1, bucket 0 for the class row/column, clamp(+-mr) + mr + 1 otherwise); they
 * are generated in-kernel from (gh, gw, mr), never read from memory.
 *   q, k, v : element (b, n, h, d) at  ptr[b*sb + n*sn + h*sh + d]  (strides in elements;
 *             the three may alias one (B, N, 3, H, 64) qkv buffer), dtype bf16 or f32
 *   tkv,tkh,tvv,tvh : (2*mr+2, 64) fp32 tables, row stride ldt elements
 *   out     : (B, N, H, 64) contiguous, same dtype as q
 *   lse     : (B, H, N) fp32       log-sum-exp of the scaled logits   (saved for backward)
 *   sp      : (B, H, 64, NP) same dtype as q: bucket sums S'^T, rows 0..31 vertical table,
 *             32..63 horizontal table, NP = cream_attn_rpe2d_padded_len(N)  (for backward; NULL: not
 *             written — a forward that no backward follows)
 * Limits: N <= 256, gh + gw + 1 <= 32, 2*mr + 2 <= 32, 16-byte aligned rows
 * (CREAM_ERR_TOO_LARGE / CREAM_ERR_BAD_ARG otherwise).  dtype: CREAM_BF16 (bf16 MFMA, fp32
 * accumulate and softmax) or CREAM_F32 (fp32 MFMA, exact fp32 products). */
int cream_attn_rpe2d_fwd(void* out, float* lse, void* sp,
                         const void* q, const void* k, const void* v,
                         int64_t sb, int64_t sn, int64_t sh,
                         const float* tkv, const float* tkh, const float* tvv, const float* tvh,
                         int ldt, int B, int H, int N, int gh, int gw, int mr,
                         float scale, int dtype, void* stream);

/* Backward of cream_attn_rpe2d_fwd (what autograd derives for multihead_super.py:135-154 and
 * the index_put of RelativePosition2D_super's table lookup, multihead_super.py:64):
 *   dq, dk, dv : gradients, element (b, n, h, d) at ptr[b*dsb + n*dsn + h*dsh + d] (may alias
 *                one (B, N, 3, H, 64) buffer), same dtype as q
 *   dtab       : (cream_attn_rpe2d_dtab_parts(B, H), 4, 32, 64) fp32, partial gradients of [tkv, tkh, tvv, tvh]
 *                (rows >= 2*mr+2 are zero): the tables are shared by every (b, h), each persistent workgroup of the
 *                dK/dV kernel accumulates over its items and writes one block; the caller sums over the first
 *                axis — a fixed-order reduction instead of atomics
 *   dlt, qe, de, delta : scratch handed from the first to the second launch:
 *                dlt (B,H,64,NP) and qe, de (B,H,NP,32) in q's dtype, delta (B,H,NP) fp32
 *   dout, out  : (B, N, H, 64) contiguous, q's dtype;  lse, sp: as written by the forward
 * Two kernels are enqueued on `stream` (dQ; then dK, dV and the table gradients).  No
 * atomics: results are bit-reproducible run to run. */
int cream_attn_rpe2d_bwd(void* dq, void* dk, void* dv, int64_t dsb, int64_t dsn, int64_t dsh,
                         float* dtab, void* dlt, void* qe, void* de, float* delta,
                         const void* dout, const void* out, const float* lse, const void* sp,
                         const void* q, const void* k, const void* v,
                         int64_t sb, int64_t sn, int64_t sh,
                         const float* tkv, const float* tkh, const float* tvv, const float* tvh,
                         int ldt, int B, int H, int N, int gh, int gw, int mr,
                         float scale, int dtype, void* stream);

/* bf16 OPERAND IMAGES of the four tables (the rows of RelativePosition2D_super's embeddings_table_v / _h,
 * multihead_super.py:22-26, as the matrix cores read them): cream_attn_rpe2d_table_image_bytes() bytes (32 KB),
 *   [key rows (64 u' x 64 d) | key^T (64 d x 64 u') | value rows | value^T],  u' = bucket of the vertical table (0..31)
 *   or 32 + bucket of the horizontal table, rows >= 2*mr+2 zero.
 * cream_attn_rpe2d_table_images builds them in one small launch; cream_adamw_step keeps them current for free when the
 * caller registers them as the bf16 copies of the four table parameters (mir = rows, mir_t = transposed at ld 64:
 * cream_amd/autoformer/block.py: BlockOperands) — the layout is exactly that of the GEMM operand copies.
 * The *_img entry points are cream_attn_rpe2d_fwd / _bwd with such an image (timg; NULL = the plain entry points):
 *   - forward, AutoFormer geometry (N = 197, 14 x 14 grid, mr = 14) in bf16: runs csrc/attn_rpe2d_fwd2.hpp — 32-key tiles with
 *     an online (lazy-maximum) softmax, two 7-wave half-workgroups per CU in ping-pong (one multiplies while the other does
 *     the element-wise / memory work), K / V by LDS-DMA; without an image (or with cream_attn_rpe2d_fwd_mode(0)) the
 *     whole-row-block kernel attn_rpe2d_fwd14 (csrc/attn_rpe2d_fwd14.hpp) runs.  Same outputs up to the rounding of the softmax numerators' reference
 *     point (both within the bf16 bounds of tests/test_attn_gpu.py).
 *   - backward (one-pass kernel): reads the image instead of building one into dlt with an extra launch.
 * cream_attn_rpe2d_fwd_mode(1 | 0): as above; < 0 queries; returns the previous value; initial: CREAM_ATTN_FWD2, else 1. */
int64_t cream_attn_rpe2d_table_image_bytes(void);
int cream_attn_rpe2d_table_images(void* img, const float* tkv, const float* tkh, const float* tvv, const float* tvh, int ldt,
                                  int mr, void* stream);
int cream_attn_rpe2d_fwd_mode(int fwd2);
int cream_attn_rpe2d_fwd_img(void* out, float* lse, void* sp,
                             const void* q, const void* k, const void* v,
                             int64_t sb, int64_t sn, int64_t sh,
                             const float* tkv, const float* tkh, const float* tvv, const float* tvh,
                             int ldt, const void* timg, int B, int H, int N, int gh, int gw, int mr,
                             float scale, int dtype, void* stream);
int cream_attn_rpe2d_bwd_img(void* dq, void* dk, void* dv, int64_t dsb, int64_t dsn, int64_t dsh,
                             float* dtab, void* dlt, void* qe, void* de, float* delta,
                             const void* dout, const void* out, const float* lse, const void* sp,
                             const void* q, const void* k, const void* v,
                             int64_t sb, int64_t sn, int64_t sh,
                             const float* tkv, const float* tkh, const float* tvv, const float* tvh,
                             int ldt, const void* timg, int B, int H, int N, int gh, int gw, int mr,
                             float scale, int dtype, void* stream);

/* The same two entry points with ATTENTION DROPOUT between the softmax and the two value-side products
 * (multihead_super.py:145 `attn = self.attn_drop(attn)`): P[i,j] -> keep[i,j] P[i,j] / (1 - dropout_p) for the P.V product and
 * the value-side bucket sums alike; lse is that of the undropped softmax.  keep is a pure function of (dropout_seed, b * H + h,
 * i, j) — a 32-bit counter-based mix (csrc/attn_common.hpp drop_keep; cream_amd/irpe_fused.py dropout_keep_mask restates it),
 * kept iff hash >= round(dropout_p 2^32) — so the backward regenerates the forward's mask from the same (dropout_p,
 * dropout_seed): no N x N mask exists in memory, and a run is reproducible from its seeds.  0 <= dropout_p < 1
 * (CREAM_ERR_BAD_ARG otherwise); dropout_p == 0 IS cream_attn_rpe2d_fwd_img / _bwd_img.  With dropout_p > 0 every geometry and
 * dtype runs the tile-streamed forward and the two-launch backward (whose score tiles are in registers where the mask applies);
 * timg is not used then. */
int cream_attn_rpe2d_fwd_drop(void* out, float* lse, void* sp,
                              const void* q, const void* k, const void* v,
                              int64_t sb, int64_t sn, int64_t sh,
                              const float* tkv, const float* tkh, const float* tvv, const float* tvh,
                              int ldt, const void* timg, int B, int H, int N, int gh, int gw, int mr,
                              float scale, float dropout_p, uint32_t dropout_seed, int dtype, void* stream);
int cream_attn_rpe2d_bwd_drop(void* dq, void* dk, void* dv, int64_t dsb, int64_t dsn, int64_t dsh,
                              float* dtab, void* dlt, void* qe, void* de, float* delta,
                              const void* dout, const void* out, const float* lse, const void* sp,
                              const void* q, const void* k, const void* v,
                              int64_t sb, int64_t sn, int64_t sh,
                              const float* tkv, const float* tkh, const float* tvv, const float* tvh,
                              int ldt, const void* timg, int B, int H, int N, int gh, int gw, int mr,
                              float scale, float dropout_p, uint32_t dropout_seed, int dtype, void* stream);

/* ---- the two ends of the supernet around the block stack (csrc/stem_tail.hip) --------------------
 * Reference: Vision_TransformerSuper.forward_features, AutoFormer/model/supernet_transformer.py:147-172
 * (patch embedding embedding_super.py:27-40, class token + position embedding :150-155, final LayerNorm and
 * token mean :166-170 for pre_norm / gp models). */

/* patches (B*gh*gw, C*ph*pw) bf16 = unfold(img (B, C, H, W) fp32): the GEMM operand of the stride = kernel conv. */
int cream_im2patch(void* patches, const float* img, int B, int C, int H, int W, int ph, int pw, void* stream);

/* x0 (B, N, E) fp32: row 0 = cls[:E] + pos[0, :E], row n = y[b, n-1, :] (bf16, (B, N-1, E)) + pos[n, :E];
 * pos may be NULL (abs_pos off); ld_pos = row stride of the position embedding (its super width). */
int cream_stem_assemble(float* x0, const void* y, const float* cls, const float* pos, int64_t ld_pos, int B, int N, int E,
                        void* stream);

/* dy (B, N-1, E) bf16 = dx0[:, 1:, :]; psum (cream_stem_bwd_chunks(B), N, E) fp32 = sums of dx0 over chunks of 16
 * images (position-embedding / class-token gradient = their sum, fixed order). */
int cream_stem_bwd_chunks(int B);
int cream_stem_bwd(void* dy, float* psum, const float* dx0, int B, int N, int E, void* stream);

/* pooled (B, E) fp32 = mean over tokens 1.. of LayerNorm(x1 + sample_scale[b] * f) (f bf16 may be NULL);
 * also writes xm (B, E) = the token mean before the affine map (-> gamma gradient), mean / rstd (B*N) and
 * uses part (B, cream_tail_chunks(N), E) as scratch.  Two launches. */
int cream_tail_chunks(int N);
int cream_tail_fwd(float* pooled, float* xm, float* part, float* mean, float* rstd, const float* x1, const void* f,
                   const float* sample_scale, const float* gamma, const float* beta, int B, int N, int E, float eps,
                   void* stream);

/* Backward of cream_tail_fwd given g = d loss / d pooled (B, E): dx (B*N, E) fp32 residual-stream gradient,
 * dx_scaled = bf16(sample_scale[b] * dx) (the gradient of f) and partial (cream_ln_partials(), E) = column
 * sums of dx_scaled (bias gradient of the projection that produced f).  gamma / beta gradients are
 * sum_b g * xm and sum_b g (caller).  The class-token rows (n = 0) of dx and dx_scaled are exactly zero.  partial
 * has cream_ln_partials() rows whatever B * N is: the rows of workgroups that had no row to walk are zeros.
 * sample_scale (NULL = 1) multiplies dx_scaled whether or not f is given: with f == NULL cream_tail_fwd has nothing
 * to scale and ignores it, while this call still writes bf16(sample_scale[b] * dx) — what the formula above says
 * (tests/test_ends_gpu.py pins both). */
int cream_tail_bwd(float* dx, void* dx_scaled, float* partial, const float* g, const float* x1, const void* f,
                   const float* mean, const float* rstd, const float* gamma, const float* sample_scale, int B, int N,
                   int E, void* stream);

/* ---- fused attention with iRPE (contextual mode) on queries, keys and values ------------------
 * Reference: RPEAttention.forward (iRPE/DeiT-with-iRPE/rpe_vision_transformer.py:68-97) between the
 * qkv and proj linears, with iRPE.forward_rpe_transpose / forward_rpe_no_transpose
 * (irpe.py:585-687) and the rpe_index gather (rpe_ops/rpe_index_cuda.cu:24-40) folded in — see
 * csrc/irpe_attn.hip for the formulas.  bf16 operands, fp32 accumulation and softmax, head_dim 64,
 * at most 64 buckets.  A table pointer (wq / wk / wv) that is NULL switches that term off. */
typedef struct cream_irpe_attn_desc {
    const void *q, *k, *v;          /* bf16; element (b, n, h, :) at ptr[b*sb + n*sn + h*sh]            */
    int64_t sb, sn, sh;
    void* out;                      /* (B, L, H, 64) bf16                                               */
    float* lse;                     /* (B, H, L)   log-sum-exp of the logits (fwd: out, bwd: in)        */
    void* sv;                       /* (B, H, NP, 64) bf16 value-side bucket sums (fwd: out, needed with wv) */
    const float *wq, *wk, *wv;      /* lookup_table_weight of rpe_q / rpe_k (H', 64, nb) and rpe_v (H', nb, 64) */
    int64_t wq_hs, wk_hs, wv_hs;    /* element stride between heads, 0 for shared_head                   */
    const uint8_t *idq, *idk, *idv;       /* (NP, NP) query-major bucket ids: idk[i][j] = bucket_k[i][j],
                                             idv[i][j] = bucket_v[i][j], idq[i][j] = bucket_q[j][i]      */
    const uint8_t *idq_t, *idk_t, *idv_t; /* the same matrices transposed (key-major), backward only     */
    int B, H, L, NP, nb;            /* NP = cream_irpe_padded_len(L)                                     */
    float scale;
    /* backward only */
    const void* dout;               /* (B, L, H, 64) bf16                                               */
    void *dq, *dk, *dv;             /* bf16; element (b, n, h, :) at ptr[b*dsb + n*dsn + h*dsh]          */
    int64_t dsb, dsn, dsh;
    float* delta;                   /* (B, H, NP) scratch                                               */
    void *lkg, *gg;                 /* (B, H, NP, 64) bf16 scratch (needed with wk / wv)                 */
    void *dlk, *dlq;                /* (B, H, NP, 64) bf16 out: bucket gradients of rpe_k / rpe_q lookups
                                       (dlq also serves as scratch inside the call: the rpe_q lookup rows of the
                                       keys live there between the pre-pass and the end of the second launch) */
    /* bias mode of rpe_q / rpe_k (irpe.py:622-624: lookup_table_bias (H', nb), no dependence on q / k): give the
     * table here INSTEAD of wq / wk; its gradient is the sum of the dlq / dlk rows over batch and tokens (caller) */
    const float *bq, *bk;
    int64_t bq_hs, bk_hs;
    /* causal != 0: key j takes part for query i only if j <= i — the additive upper-triangular -inf mask of the text
     * towers (TinyCLIP/src/open_clip/model.py:756-762) without an (L, L) tensor; 0: full attention */
    int32_t causal, reserved;
    /* attention dropout (rpe_vision_transformer.py:86, multihead_super.py:145 `attn = self.attn_drop(attn)`):
     * P[i,j] -> keep[i,j] P[i,j] / (1 - dropout_p) after the softmax, for the value product and the value-side
     * bucket sums alike; keep is a pure function of (dropout_seed, b, h, i, j) — the SAME seed must be given to
     * cream_irpe_attn_bwd.  0 <= dropout_p < 1 (0: none); L <= 65535 with dropout. */
    float dropout_p;
    uint32_t dropout_seed;
} cream_irpe_attn_desc;

int cream_irpe_padded_len(int L);

/* int32 (Lq, Lk) bucket ids (irpe.py:523-583) -> zero-padded uint8 (NP, NP) holding 2 * id (the byte
 * offset of the bucket in a bf16 lookup row; ids < 64); transpose != 0 converts the transposed table (dst row j
 * = column j of ids).  Done once per (table, device) by the caller.  The matrix is an OPAQUE operand of the two
 * calls below: inside every 32-byte group of a row (one streamed tile of 32 partners) the bytes are in the order
 * the lanes of the kernels read them (byte 16 g + r = partner (r & 3) + 8 (r >> 2) + 4 g of the tile), so that a
 * lane's 16 ids of a tile are one 16-byte load. */
int cream_irpe_bucket_bytes(uint8_t* dst, const int32_t* ids, int Lq, int Lk, int NP, int transpose, void* stream);

/* out, lse (and sv) from q, k, v.  One launch. */
int cream_irpe_attn_fwd(const cream_irpe_attn_desc* d, void* stream);

/* dq, dk, dv and the bucket-gradient rows dlk, dlq from dout (+ out, lse of the forward).  Two launches
 * (queries own lanes; keys own lanes) behind a small pre-pass when wq is given ((k * scale) Wq rows of all keys);
 * no global atomics. */
int cream_irpe_attn_bwd(const cream_irpe_attn_desc* d, void* stream);

/* Per-(b,h) table gradient  out[b*H+h][a][c] = mul * sum_n X[b,n,h][a] * Y[b,n,h][c]  (64 x 64 fp32):
 *   d lookup_table_weight(rpe_k) = (scale q)^T dlk, (rpe_q) = (scale k)^T dlq, (rpe_v) = sv^T dout;
 * the caller sums over b (and h for shared tables).  X, Y bf16 with element strides (sb, sn, sh). */
int cream_irpe_table_grad(float* out, const void* x, int64_t xsb, int64_t xsn, int64_t xsh, const void* y, int64_t ysb,
                          int64_t ysn, int64_t ysh, int B, int H, int L, float mul, void* stream);

/* ---- fused Mini-DeiT attention: head-mixing 1x1 convolutions before (wl) and after (ww) the softmax ------------
 * MiniAttention.forward with use_transform (MiniViT/Mini-DeiT/mini_vision_transformer.py:84-114) between the qkv and
 * proj linears — see csrc/mini_attn.hip for the formulas:
 *     S_h = (s q_h) k_h^T + rpe_k lookups,  S'_o = sum_h wl[o,h] S_h,  P_o = softmax(S'_o),  P'_o = sum_h ww[o,h] P_h,
 *     O_o = P'_o v_o.
 * bf16 operands, fp32 accumulation, head_dim 64, 1 <= H <= 12, L <= 2048, contextual rpe on k with at most 64 buckets
 * (wk == NULL: none).  Fields named as in cream_irpe_attn_desc mean the same; lse is the log-sum-exp of the MIXED
 * logits S'.  Anything else (H > 12, head_dim != 64, nb > 64, a missing wl or ww) returns CREAM_ERR_BAD_ARG before any
 * HIP call.  Nothing of size L^2 is written; no global atomics: the two H x H weight gradients come as one partial
 * per workgroup, (B * NP / 32, H, H) fp32 each, [out][in] like the weights, which the caller sums over the first axis. */
typedef struct cream_mini_attn_desc {
    const void *q, *k, *v;          /* bf16; element (b, n, h, :) at ptr[b*sb + n*sn + h*sh]            */
    int64_t sb, sn, sh;
    void* out;                      /* (B, L, H, 64) bf16 (fwd only: the backward does not read it)    */
    float* lse;                     /* (B, H, L) (fwd: out, bwd: in)                                     */
    const float* wk;                /* lookup_table_weight of rpe_k (H', 64, nb) or NULL                 */
    int64_t wk_hs;                  /* element stride between heads, 0 for shared_head                   */
    const uint8_t *idk, *idk_t;     /* (NP, NP) cream_irpe_bucket_bytes matrices, query- / key-major (bwd) */
    const float *wl, *ww;           /* (H, H) fp32, [out][in]: conv_l / conv_w weight[:, :, 0, 0]        */
    int32_t B, H, L, NP, nb, head_dim;
    float scale;
    int32_t reserved;
    /* backward only */
    const void* dout;               /* (B, L, H, 64) bf16                                               */
    void *dq, *dk, *dv;             /* bf16; element (b, n, h, :) at ptr[b*dsb + n*dsn + h*dsh]          */
    int64_t dsb, dsn, dsh;
    float* delta;                   /* (B, H, NP) scratch                                               */
    void *lkg, *dlk;                /* (B, H, NP, 64) bf16: scratch / out (bucket gradients of the rpe_k lookups;
                                       d lookup_table_weight = cream_irpe_table_grad(q, dlk, mul = scale)) */
    float *dwl_part, *dww_part;     /* (B * NP / 32, H, H) fp32 out                                      */
} cream_mini_attn_desc;

/* out and lse from q, k, v.  One launch (two passes over the keys inside). */
int cream_mini_attn_fwd(const cream_mini_attn_desc* d, void* stream);

/* dq, dk, dv, the dlk rows and the partials of d wl / d ww from dout and lse.  2 + ceil(H / 4) launches. */
int cream_mini_attn_bwd(const cream_mini_attn_desc* d, void* stream);

/* ---- fused (shifted-)window attention of Swin / Mini-Swin ---------------------------------------------------------
 * WindowAttention.forward between the qkv and proj linears, with the cyclic shift, window partition and reverse of
 * SwinTransformerBlock.forward_feature in the addressing (MiniViT/Mini-Swin/models/swin_transformer_minivit.py:109-147,
 * :284-323) — see csrc/window_attn.hip for the formulas:
 *     S_h = (s q_h) k_h^T + table[rel(i,j), h],  S'_o = sum_h wl[o,h] S_h + bl[o] (+ mask in {0, -100}),
 *     P_o = softmax(S'_o),  P'_o = sum_h ww[o,h] P_h + bw[o],  O_o = P'_o v_o.
 * q, k, v are the projection of the UNSHIFTED, UNPARTITIONED (Hs x Ws) map, token n = y * Ws + x; out has the same token
 * order.  Window (wy, wx), local (iy, ix) is token ((wy w + iy + shift) mod Hs, (wx w + ix + shift) mod Ws).  mask_shift
 * m > 0 adds -100 between tokens of different regions of the shifted frame (three slices per axis: [0, Hs - w),
 * [Hs - w, Hs - m), [Hs - m, Hs)); the reference applies a block's mask whether or not the repeat rolls the map, hence
 * two arguments.  bf16 operands, fp32 accumulation; head_dim 32, square windows with w * w <= 64, Hs and Ws multiples of
 * w, shift < w, mask_shift < w; wl, bl, ww, bw all NULL (no head transforms, 1 <= H <= 32) or all given (1 <= H <= 16).
 * Anything else returns CREAM_ERR_BAD_ARG before any HIP call; B == 0 is a no-op.  Nothing of size N^2 per window is
 * written; no global atomics: the backward's parameter gradients come as one partial per workgroup of its persistent
 * grid, (part_blocks, part_size) fp32 = [d table ((2w-1)^2, H) | d wl (H, H) | d ww (H, H) | d bl (H) | d bw (H)] (the
 * last four only with head transforms), which the caller sums over the first axis. */
typedef struct cream_window_attn_desc {
    const void *q, *k, *v;          /* bf16; element (b, n, h, :) at ptr[b*sb + n*sn + h*sh]                 */
    int64_t sb, sn, sh;
    void* out;                      /* (B, Hs*Ws, H, 32) bf16 (fwd only)                                   */
    float* lse;                     /* (B * nW, H, 64): log-sum-exp of the mixed, masked logits (fwd: out, bwd: in) */
    const float* table;             /* ((2w-1)^2, H) fp32                                                  */
    const float *wl, *bl, *ww, *bw; /* (H, H) [out][in] and (H) fp32, or all NULL                          */
    int32_t B, H, Hs, Ws, w, shift, mask_shift, head_dim;
    float scale;
    int32_t part_blocks;            /* bwd: cream_window_attn_blocks(d), the first axis of `part`           */
    /* backward only */
    const void* dout;               /* (B, Hs*Ws, H, 32) bf16                                              */
    void *dq, *dk, *dv;             /* bf16; element (b, n, h, :) at ptr[b*dsb + n*dsn + h*dsh]             */
    int64_t dsb, dsn, dsh;
    float* delta;                   /* (B * nW, H, 64) scratch                                             */
    float* part;                    /* (part_blocks, cream_window_attn_part_size(H, w, mixed)) fp32 out     */
} cream_window_attn_desc;

/* The argument check of the calls below alone (backward != 0: of cream_window_attn_bwd, except part_blocks' value):
 * CREAM_OK or the error code.  Pure host arithmetic. */
int cream_window_attn_check(const cream_window_attn_desc* d, int backward);

/* Floats per workgroup partial, or CREAM_ERR_BAD_ARG.  Pure host arithmetic. */
int cream_window_attn_part_size(int H, int w, int mixed);

/* Workgroups of the persistent grids for this descriptor's shape (B, H, Hs, Ws, w, head transforms or not; from
 * cream_cu_count(); the data pointers are not looked at), 0 when B == 0, or an error code. */
int cream_window_attn_blocks(const cream_window_attn_desc* d);

/* out and lse from q, k, v.  One launch. */
int cream_window_attn_fwd(const cream_window_attn_desc* d, void* stream);

/* dq, dk, dv and the partials of the parameter gradients from dout and lse.  Two launches. */
int cream_window_attn_bwd(const cream_window_attn_desc* d, void* stream);

/* ---- fused (shifted-)window attention for windows of 9x9 .. 14x14 (csrc/window_attn_large.hip) ---------------------
 * WindowAttention.forward of AutoFormerV2 / S3 between the qkv and proj linears (AutoFormerV2/model/SSS.py:106-137), with
 * the geometry of cream_window_attn_desc in the addressing:
 *     S_h = (s q_h) k_h^T + table[rel(i,j), h] (+ mask in {0, -100}),  P_h = softmax(S_h),  O_h = P_h v_h.
 * bf16 operands, fp32 accumulation; head_dim 32, 1 <= H <= 32 independent heads (no head transforms), square windows with
 * 9 <= w <= 14, Hs and Ws multiples of w, shift < w, mask_shift < w.  Anything else returns CREAM_ERR_BAD_ARG before any
 * HIP call; B == 0 is a no-op.  NP = w * w rounded up to a multiple of 32.  Nothing of size N^2 per window is written; no
 * global atomics: d table comes as (part_blocks, (2w-1)^2, H) fp32 partials, every entry written once, which the caller
 * sums over the first axis. */
typedef struct cream_window_attn_large_desc {
    const void *q, *k, *v;          /* bf16; element (b, n, h, :) at ptr[b*sb + n*sn + h*sh]                 */
    int64_t sb, sn, sh;
    void* out;                      /* (B, Hs*Ws, H, 32) bf16 (fwd only)                                   */
    float* lse;                     /* (B * nW, H, NP): log-sum-exp of the masked logits (fwd: out, bwd: in) */
    const float* table;             /* ((2w-1)^2, H) fp32                                                  */
    int32_t B, H, Hs, Ws, w, shift, mask_shift, head_dim;
    float scale;
    int32_t part_blocks;            /* bwd: cream_window_attn_large_blocks(d), the first axis of `part`     */
    /* backward only */
    const void* dout;               /* (B, Hs*Ws, H, 32) bf16                                              */
    void *dq, *dk, *dv;             /* bf16; element (b, n, h, :) at ptr[b*dsb + n*dsn + h*dsh]             */
    int64_t dsb, dsn, dsh;
    float* delta;                   /* (B * nW, H, NP) fp32 out: sum_j P dP of every query                 */
    float* part;                    /* (part_blocks, cream_window_attn_large_part_size(H, w)) fp32 out      */
} cream_window_attn_large_desc;

/* The argument check of the calls below alone (backward != 0: of cream_window_attn_large_bwd, except part_blocks'
 * value): CREAM_OK or the error code.  Pure host arithmetic. */
int cream_window_attn_large_check(const cream_window_attn_large_desc* d, int backward);

/* Floats per partial, (2w-1)^2 H, or CREAM_ERR_BAD_ARG.  Pure host arithmetic. */
int cream_window_attn_large_part_size(int H, int w);

/* Partials of d table for this descriptor's shape (B, H, Hs, Ws, w): the persistent grids have this many workgroups per
 * head (from cream_cu_count(); the data pointers are not looked at), 0 when B == 0, or an error code. */
int cream_window_attn_large_blocks(const cream_window_attn_large_desc* d);

/* out and lse from q, k, v.  One launch. */
int cream_window_attn_large_fwd(const cream_window_attn_large_desc* d, void* stream);

/* dq, dk, dv, delta and the partials of d table from dout and lse.  Two launches. */
int cream_window_attn_large_bwd(const cream_window_attn_large_desc* d, void* stream);

/* ---- fused head-mixing (shifted-)window attention for windows of 9x9 .. 12x12 (csrc/window_attn_mix_large.hip) --------
 * The attention of Mini-Swin at window 12 (Mini-Swin-B at 384) between the qkv and proj linears: the formulas, the geometry
 * and the layout of the partials of cream_window_attn_desc with head transforms, on key rows of 3 to 5 tiles (a two-pass
 * softmax).  bf16 operands, fp32 accumulation; head_dim 32, square windows with 9 <= w <= 12, Hs and Ws multiples of w,
 * shift < w, mask_shift < w; wl, bl, ww, bw all given, 1 <= H <= 16.  Anything else (32 heads included) returns
 * CREAM_ERR_BAD_ARG before any HIP call; B == 0 is a no-op.  lse and delta are (B * nW, H, NP), NP = w * w rounded up to a
 * multiple of 32.  Nothing of size N^2 per window is written; no global atomics: the backward's parameter gradients come as
 * one partial per workgroup of its persistent grid, (part_blocks, part_size) fp32 = [d table ((2w-1)^2, H) | d wl (H, H) |
 * d ww (H, H) | d bl (H) | d bw (H)], which the caller sums over the first axis. */
typedef cream_window_attn_desc cream_window_attn_mix_large_desc;    /* the same fields; lse and delta (B * nW, H, NP) */

/* The argument check of the calls below alone (backward != 0: of cream_window_attn_mix_large_bwd, except part_blocks'
 * value): CREAM_OK or the error code.  Pure host arithmetic. */
int cream_window_attn_mix_large_check(const cream_window_attn_mix_large_desc* d, int backward);

/* Floats per workgroup partial, (2w-1)^2 H + 2 H^2 + 2 H = cream_window_attn_part_size(H, w, 1)'s formula, or
 * CREAM_ERR_BAD_ARG.  Pure host arithmetic. */
int cream_window_attn_mix_large_part_size(int H, int w);

/* Workgroups of the backward's query launch for this descriptor's shape (B, H, Hs, Ws, w; from cream_cu_count(); the data
 * pointers other than wl, bl, ww, bw are not looked at), 0 when B == 0, or an error code. */
int cream_window_attn_mix_large_blocks(const cream_window_attn_mix_large_desc* d);

/* out and lse from q, k, v.  One launch. */
int cream_window_attn_mix_large_fwd(const cream_window_attn_mix_large_desc* d, void* stream);

/* dq, dk, dv, delta and the partials of the parameter gradients from dout and lse.  Two launches. */
int cream_window_attn_mix_large_bwd(const cream_window_attn_mix_large_desc* d, void* stream);

/* ---- fused window attention for windows of 15x15 .. 32x32 (csrc/window_attn_xl.hip) ----------------------------------
 * The attention of a TinyViT block at high resolution (TinyViT/models/tiny_vit.py:216-286, windows of 16, 24 and 32) between
 * the qkv and proj linears, with the window partition in the addressing:
 *     S_h = (s q_h) k_h^T + table[rel(i,j), h],  P_h = softmax(S_h),  O_h = P_h v_h.
 * The conventions of cream_window_attn_large_desc; keys and values stream through LDS instead of staying there.  bf16
 * operands, fp32 accumulation; head_dim 32, 1 <= H <= 32 independent heads, square windows with 15 <= w <= 32, Hs and Ws
 * multiples of w, shift == mask_shift == 0 (no shifted window is implemented at these sizes).  Anything else returns
 * CREAM_ERR_BAD_ARG before any HIP call; B == 0 is a no-op.  NP = w * w rounded up to a multiple of 32.  Nothing of size N^2
 * per window is written; no global atomics: d table comes as (part_blocks, (2w-1)^2, H) fp32 partials, every entry written
 * once, which the caller sums over the first axis. */
typedef cream_window_attn_large_desc cream_window_attn_xl_desc;     /* the same fields; shift and mask_shift must be 0 */

/* The argument check of the calls below alone (backward != 0: of cream_window_attn_xl_bwd, except part_blocks' value):
 * CREAM_OK or the error code.  Pure host arithmetic. */
int cream_window_attn_xl_check(const cream_window_attn_xl_desc* d, int backward);

/* Floats per partial, (2w-1)^2 H, or CREAM_ERR_BAD_ARG.  Pure host arithmetic. */
int cream_window_attn_xl_part_size(int H, int w);

/* Partials of d table for this descriptor's shape (B, H, Hs, Ws, w): the persistent grids have this many workgroups per
 * head (from cream_cu_count(); the data pointers are not looked at), 0 when B == 0, or an error code. */
int cream_window_attn_xl_blocks(const cream_window_attn_xl_desc* d);

/* out and lse from q, k, v.  One launch. */
int cream_window_attn_xl_fwd(const cream_window_attn_xl_desc* d, void* stream);

/* dq, dk, dv, delta and the partials of d table from dout and lse.  Two launches. */
int cream_window_attn_xl_bwd(const cream_window_attn_xl_desc* d, void* stream);

/* ---- depthwise 3 x 3 convolution on the token layout (csrc/token_dwconv.hip) -----------------------------------------
 * The local convolution of a TinyViT block (TinyViT/models/tiny_vit.py:333-335, :374-376) without the transposes to NCHW and
 * back: x (B, Hs*Ws, C) contiguous, token n = i * Ws + j; stride 1, zero padding 1:
 *     y[b, i, j, c]  = bias[c] + sum_{di, dj} w[c, di, dj] x[b, i + di - 1, j + dj - 1, c]
 *     dx[b, i, j, c] = sum_{di, dj} w[c, di, dj] dy[b, i - di + 1, j - dj + 1, c]
 *     dw[c, di, dj]  = sum_{b, i, j} dy[b, i, j, c] x[b, i + di - 1, j + dj - 1, c],   dbias[c] = sum_{b, i, j} dy[b, i, j, c]
 * x, y, dy, dx in `dtype` (CREAM_BF16 or CREAM_F32), taps, bias and the partials fp32; fp32 accumulation, bias first, then
 * the taps in row-major order.  C a multiple of 8, B, Hs, Ws >= 1, every base 16-byte aligned (bias: 4); anything else
 * returns CREAM_ERR_BAD_ARG (CREAM_ERR_BAD_DTYPE) before any HIP call.  No atomics: dw and dbias come as (part_blocks,
 * cream_token_dwconv3_part_size(C)) fp32 partials [dw (C, 9) | dbias (C)], every entry written once, which the caller sums
 * over the first axis. */
typedef struct cream_token_dwconv3_desc {
    const void* x;                  /* (B, Hs*Ws, C)                                                        */
    const float* w;                 /* (C, 1, 3, 3) fp32 contiguous                                         */
    const float* bias;              /* (C) fp32 or NULL (fwd only)                                          */
    void* y;                        /* (B, Hs*Ws, C) (fwd only)                                             */
    int32_t B, Hs, Ws, C, dtype;
    int32_t part_blocks;            /* bwd: cream_token_dwconv3_blocks(d), the first axis of `part`         */
    /* backward only */
    const void* dy;                 /* (B, Hs*Ws, C)                                                        */
    void* dx;                       /* (B, Hs*Ws, C)                                                        */
    float* part;                    /* (part_blocks, 10 C) fp32 out                                         */
} cream_token_dwconv3_desc;

/* Floats per partial, 10 C, or CREAM_ERR_BAD_ARG.  Pure host arithmetic. */
int cream_token_dwconv3_part_size(int C);

/* Workgroups along the token axis of the gradient launch for this descriptor's shape (B, Hs, Ws, C, dtype; from
 * cream_cu_count(); the data pointers are not looked at), or an error code. */
int cream_token_dwconv3_blocks(const cream_token_dwconv3_desc* d);

/* y from x, w and bias.  One launch. */
int cream_token_dwconv3_fwd(const cream_token_dwconv3_desc* d, void* stream);

/* dx and the partials of dw and dbias from dy and x.  Two launches. */
int cream_token_dwconv3_bwd(const cream_token_dwconv3_desc* d, void* stream);

/* ---- depthwise 7 x 7 convolution on the token layout, residual fused (csrc/token_dwconv7.hip) ------------------------
 * The local convolution of a Mini-Swin block repeat (MiniViT/Mini-Swin/models/swin_transformer_minivit.py:328-332) without
 * the transposes to NCHW and back: x (B, Hs*Ws, C) contiguous, token n = i * Ws + j; stride 1, zero padding 3, r = residual:
 *     y[b, i, j, c]  = bias[c] + sum_{di, dj} w[c, di, dj] x[b, i + di - 3, j + dj - 3, c]   (+ x[b, i, j, c] if r)
 *     dx[b, i, j, c] = sum_{di, dj} w[c, di, dj] dy[b, i - di + 3, j - dj + 3, c]            (+ dy[b, i, j, c] if r)
 *     dw[c, di, dj]  = sum_{b, i, j} dy[b, i, j, c] x[b, i + di - 3, j + dj - 3, c],   dbias[c] = sum_{b, i, j} dy[b, i, j, c]
 * x, y, dy, dx in `dtype` (CREAM_BF16 or CREAM_F32), taps, bias and the partials fp32; fp32 accumulation, bias first, then
 * the taps in row-major order of the input offset, then the residual.  C a multiple of 8, B, Hs, Ws >= 1, residual 0 or 1,
 * every base 16-byte aligned (bias: 4); anything else returns CREAM_ERR_BAD_ARG (CREAM_ERR_BAD_DTYPE) before any HIP call.
 * No atomics: dw and dbias come as (part_blocks, cream_token_dwconv7_part_size(C)) fp32 partials [dw (C, 49) | dbias (C)],
 * every entry written once, which the caller sums over the first axis. */
typedef struct cream_token_dwconv7_desc {
    const void* x;                  /* (B, Hs*Ws, C)                                                        */
    const float* w;                 /* (C, 1, 7, 7) fp32 contiguous                                         */
    const float* bias;              /* (C) fp32 or NULL (fwd only)                                          */
    void* y;                        /* (B, Hs*Ws, C) (fwd only)                                             */
    int32_t B, Hs, Ws, C, dtype;
    int32_t part_blocks;            /* bwd: cream_token_dwconv7_blocks(d), the first axis of `part`         */
    int32_t residual;               /* 1: y += x, dx += dy                                                  */
    /* backward only */
    const void* dy;                 /* (B, Hs*Ws, C)                                                        */
    void* dx;                       /* (B, Hs*Ws, C)                                                        */
    float* part;                    /* (part_blocks, 50 C) fp32 out                                         */
} cream_token_dwconv7_desc;

/* Floats per partial, 50 C, or CREAM_ERR_BAD_ARG.  Pure host arithmetic. */
int cream_token_dwconv7_part_size(int C);

/* Workgroups along the tile axis of every launch for this descriptor's shape (B, Hs, Ws, C, dtype; from cream_cu_count();
 * the data pointers are not looked at), or an error code. */
int cream_token_dwconv7_blocks(const cream_token_dwconv7_desc* d);

/* y from x, w and bias.  One launch. */
int cream_token_dwconv7_fwd(const cream_token_dwconv7_desc* d, void* stream);

/* dx and the partials of dw and dbias from dy and x.  Two launches. */
int cream_token_dwconv7_bwd(const cream_token_dwconv7_desc* d, void* stream);

/* ---- EfficientViT's cascaded group attention, inference (csrc/cga_attn.hip) ------------------------------------------
 * What CascadedGroupAttention.forward (EfficientViT/classification/model/efficientvit.py:159-180) computes between its input
 * and the ReLU in front of `proj`, BatchNorm folded, for every w x w window of the map in one launch.  With Cg = C / h and
 * x_i the i-th group of Cg channels, head i = 0 .. h - 1 in sequence:
 *     feat_in_i = x_i (i = 0)  |  feat_{i-1} + x_i
 *     [q | k | v] = feat_in_i W_i^T + b_i                    q, k: 16 wide, v: Cg wide
 *     q' = depthwise k_i x k_i convolution of q inside the window (zero padding) + bias
 *     feat_i = softmax(scale q' k^T + ab_i) v                out[.., i Cg : (i + 1) Cg] = feat_i  (relu: max(feat_i, 0))
 * Rounding: feat_in, q, k, v, q' and feat_i are bf16 (fp32 accumulation, then bias, then one rounding); logits, softmax and the
 * row sum fp32; the probabilities enter the last product as bf16(exp(l - max)), the division by the fp32 row sum comes after
 * it.  The stored pre-ReLU feat_i is the value head i + 1 reads.
 * Ranges: Cg in {16, 32, .., 112}, 1 <= h <= 4, 1 <= w <= 8, k_i in {1, 3, 5, 7}, Hs and Ws multiples of w.  x, wqkv, bqkv and out
 * 16-byte aligned, the strides of x multiples of 8 elements with xsx >= h Cg; anything else returns CREAM_ERR_BAD_ARG before
 * any HIP call.  One workgroup per window (not persistent), no atomics, no scratch. */
typedef struct cream_cga_desc {
    const void* x;                  /* bf16, element (b, y, x, c) at b xsb + y xsy + x xsx + c                 */
    int64_t xsb, xsy, xsx;          /* in elements                                                             */
    const void* wqkv;               /* bf16 (h, 32 + Cg, KP): rows [q | k | v], KP = Cg rounded up to 32, zeros past Cg */
    const float* bqkv;              /* (h, 32 + Cg)                                                            */
    const float* dw;                /* the taps (16, k_i, k_i) of head 0, 1, .. one after the other            */
    const float* dwb;               /* (h, 16)                                                                 */
    const float* ab;                /* (h, w^2, w^2): attention_biases[:, attention_bias_idxs]                 */
    void* out;                      /* bf16 (B, Hs, Ws, h Cg) contiguous                                       */
    int32_t B, Hs, Ws, w, h, Cg, relu;
    int32_t ks[4];                  /* k_i                                                                     */
    float scale;
} cream_cga_desc;

/* CREAM_OK when cream_cga_attn_fwd would launch for this descriptor, its error code otherwise.  Pure host arithmetic. */
int cream_cga_attn_check(const cream_cga_desc* d);

/* out from x and the folded operands.  One launch. */
int cream_cga_attn_fwd(const cream_cga_desc* d, void* stream);

/* ---- EfficientViT's depthwise 3 x 3 + FFN pair and proj + residual on the token layout, inference (csrc/evit_ffn.hip) ----
 * What  ffn(dw(x))  of an EfficientViTBlock (EfficientViT/classification/model/efficientvit.py:263-282: two Residuals, around a
 * depthwise 3 x 3 Conv2d_BN and around FFN = pw1 -> ReLU -> pw2, :92-101) computes in eval mode, BatchNorm folded, one launch:
 *     y1  = x + sum_k taps[k] x(y + k / 3 - 1, x + k % 3 - 1) + dwb          zero outside the token's own map
 *     out = y1 + W2 relu(W1 y1 + b1) + b2
 * Rounding: the taps, dwb and y1 fp32; the first product reads bf16(y1), accumulates in fp32, then + b1, ReLU, one rounding to
 * bf16; the second product accumulates in fp32 on top of the fp32 y1; out = bf16(.. + b2).  y1 and the hidden activation never
 * reach memory.  Ranges: 16 <= C <= 384 in steps of 16, 32 <= Ch <= 768 in steps of 32, B, H, W >= 1.  Every pointer 16-byte
 * aligned.  x is a strided view with channel stride 1 and batch / row / column strides that are multiples of 8 elements with
 * xsx >= C: a token tensor, a slice of a larger buffer, a channels-last NCHW tensor.  The checks return, in this order:
 * CREAM_ERR_BAD_SHAPE (C, Ch, B, H, W), CREAM_ERR_TOO_LARGE (B H W > 2^31 - 65), CREAM_ERR_BAD_ARG (a null or misaligned
 * pointer), CREAM_ERR_CHANNEL_STRIDE, CREAM_ERR_BAD_STRIDE — before any HIP call.  One workgroup per 64 consecutive tokens (not
 * persistent), no atomics, no scratch. */
typedef struct cream_evit_dwffn_desc {
    const void* x;                  /* bf16, element (b, y, x, c) at b xsb + y xsy + x xsx + c xsc              */
    int64_t xsb, xsy, xsx, xsc;     /* in elements; xsc must be 1                                              */
    const float* taps;              /* (9, C): tap k = 3 ky + kx of channel c at k C + c                       */
    const float* dwb;               /* (C)                                                                     */
    const void* w1;                 /* bf16 (Ch, KP), KP = C rounded up to 32, zeros past C                    */
    const float* b1;                /* (Ch)                                                                    */
    const void* w2;                 /* bf16 (C, Ch)                                                            */
    const float* b2;                /* (C)                                                                     */
    void* out;                      /* bf16 (B, H, W, C) contiguous                                            */
    int32_t B, H, W, C, Ch;
} cream_evit_dwffn_desc;

/* CREAM_OK when cream_evit_dwffn_fwd would launch for this descriptor, its error code otherwise.  Pure host arithmetic. */
int cream_evit_dwffn_check(const cream_evit_dwffn_desc* d);

/* out from x and the folded operands.  One launch. */
int cream_evit_dwffn_fwd(const cream_evit_dwffn_desc* d, void* stream);

/* out = res + W a + b: the 1 x 1 Conv2d_BN `proj` of CascadedGroupAttention (:127-128) on the output of cream_cga_attn_fwd
 * (which applies the ReLU in front of it) with the mixer's Residual folded in.  out = bf16(fp32(res) + b + fp32 products).
 * 16 <= Cin, Cout <= 384 in steps of 16; a and res are strided views under the rules of x above; the same codes. */
typedef struct cream_evit_pw_desc {
    const void* a;                  /* bf16 (B, H, W, Cin) view                                                */
    int64_t asb, asy, asx, asc;
    const void* res;                /* bf16 (B, H, W, Cout) view                                               */
    int64_t rsb, rsy, rsx, rsc;
    const void* w;                  /* bf16 (Cout, KP), KP = Cin rounded up to 32, zeros past Cin              */
    const float* b;                 /* (Cout)                                                                  */
    void* out;                      /* bf16 (B, H, W, Cout) contiguous                                         */
    int32_t B, H, W, Cin, Cout;
} cream_evit_pw_desc;

int cream_evit_pw_residual_check(const cream_evit_pw_desc* d);

int cream_evit_pw_residual_fwd(const cream_evit_pw_desc* d, void* stream);

/* ---- the relation losses of the Mini-Swin distillation step (csrc/distill_loss.hip) -------------------------------
 * cal_relation_loss and cal_hidden_relation_loss of MiniViT/Mini-Swin/main.py:39-57 and :66-77, each with the gradient
 * with respect to the student in the same call.  No atomics: one fp32 partial of the (already scaled) loss per workgroup,
 * which the caller sums; every gradient element is written once.  Nothing of size N^2 per window or L^2 per image is
 * written.
 *
 * Relation loss: per window of w * w <= 64 tokens, per channel group of Ar and per ordered pair (i, j) of {q, k, v}
 *     A_s = X_i X_j^T / sqrt(Cs / Ar),  A_t = Y_i Y_j^T / sqrt(Ct / Ar),  loss += coef * sum_rows -softmax(A_t) . log_softmax(A_s)
 *     G_ij = coef (softmax(A_s) - softmax(A_t)):  dX_i += G_ij X_j / sqrt(Cs / Ar),  dX_j += G_ij^T X_i / sqrt(Cs / Ar).
 * A side is B maps of Hs x Ws tokens (token n = y * Ws + x, channel stride 1), partitioned into w x w windows after a cyclic
 * shift as in cream_window_attn_desc; windows that are already partitioned are B * nW maps of w x w.  Both sides have the
 * same w and the same number of windows, C / Ar is a multiple of 32 on both; everything else may differ. */
typedef struct cream_relation_side {
    const void *q, *k, *v;          /* bf16; element (b, n, c) at ptr[b*sb + n*sn + c]                      */
    int64_t sb, sn;
    int32_t B, C, Hs, Ws, w, shift;
} cream_relation_side;

typedef struct cream_relation_desc {
    cream_relation_side s, t;       /* student, teacher                                                    */
    int32_t Ar, want_grad;
    float coef;                     /* 1 / (rows * 9 * layers), rows = windows * Ar * w * w                */
    int32_t part_blocks;            /* cream_relation_loss_blocks(d), the length of `part`                 */
    float* part;
    void *dq, *dk, *dv;             /* want_grad: bf16; element (b, n, c) at ptr[b*dsb + n*dsn + c]         */
    int64_t dsb, dsn;
} cream_relation_desc;

/* The argument check of cream_relation_loss alone (except part_blocks' value).  Pure host arithmetic. */
int cream_relation_loss_check(const cream_relation_desc* d);

/* Workgroups of the persistent grid for this descriptor's shapes and want_grad (from cream_cu_count(); the data pointers
 * are not looked at), 0 for an empty batch, or an error code. */
int cream_relation_loss_blocks(const cream_relation_desc* d);

/* part, and with want_grad dq, dk, dv.  One launch. */
int cream_relation_loss(const cream_relation_desc* d, void* stream);

/* Hidden relation loss of hidden states s (B, L, Cs) and t (B, L, Ct), contiguous, fp32 or bf16 each:
 *     S^ = s / max(|s|, 1e-12) per row (norms in fp32), T^ likewise,  D = S^ S^^T - T^ T^^T,  loss = coef * sum D^2,
 *     ds = (g - S^ (S^ . g)) / max(|s|, 1e-12)  with  g_i = 4 coef sum_j D_ij S^_j,   in s's dtype.
 * Scratch: sn (B, L, P(Cs)) and tn (B, L, P(Ct)) bf16 with P = cream_hidden_relation_padded, s_rinv and t_rinv (B, L) fp32,
 * with want_grad g (B, L, P(Cs)) fp32; part: cream_hidden_relation_parts(B, L) floats.  Up to four launches. */
typedef struct cream_hidden_relation_desc {
    const void *s, *t;
    int32_t s_dtype, t_dtype, B, L, Cs, Ct, want_grad;
    float coef;                     /* 49 / (B * L * L * layers)                                           */
    void *sn, *tn;
    float *s_rinv, *t_rinv, *g, *part;
    void* ds;                       /* want_grad: (B, L, Cs) in s_dtype                                    */
} cream_hidden_relation_desc;

int cream_hidden_relation_check(const cream_hidden_relation_desc* d);
int cream_hidden_relation_padded(int C);
int cream_hidden_relation_parts(int B, int L);
int cream_hidden_relation_loss(const cream_hidden_relation_desc* d, void* stream);

/* ---- fused iRPE attention, generalised: 32- or 64-wide heads, up to 128 buckets, key padding mask -------------
 * The same operator as cream_irpe_attn_fwd / _bwd (same formulas, launches and conventions; csrc/irpe_attn_x.hip),
 * for the callers those entry points refuse: DETR-with-iRPE's encoder self-attention (d_model 256 / 8 heads = 32,
 * `--enc_rpe2d rpe-2.0-product-ctx-1-k` = 81 buckets, `key_padding_mask` on every call; models/transformer.py,
 * rpe_attention_function.py:349-357) and every iRPE configuration with 64 < nb <= 128 buckets on k.
 * `base` is a cream_irpe_attn_desc with the SAME meaning of every field, except that wherever that block says 64:
 *   - the head width (q / k / v / out / dout / dq / dk / dv rows, the D of the tables (H', D, nb) / (H', nb, D)) is
 *     head_dim;
 *   - the width of the bucket-indexed side rows sv, lkg, gg, dlk, dlq — (B, H, NP, row_width) bf16 — is row_width,
 *     and base.nb <= row_width.  Columns nb .. row_width - 1 of sv / dlk / dlq come out zero.
 * Implemented: head_dim 32 | 64; row_width 64 with every subset of rpe on q / k / v (contextual or bias mode, shared
 * or per-head tables), row_width 128 with rpe on k ALONE (wk or bk given; wq, bq, wv NULL).  Everything else —
 * head_dim 48, nb > row_width, row_width 128 with a q or v table — returns CREAM_ERR_BAD_ARG and launches nothing.
 * The bucket byte matrices are those of cream_irpe_bucket_bytes (they hold 2 * id: ids up to 127 fit). */
typedef struct cream_irpe_attn2_desc {
    cream_irpe_attn_desc base;
    int32_t head_dim;               /* 32 | 64                                                            */
    int32_t row_width;              /* 64 | 128                                                           */
    /* key padding mask: (B, L) bytes, element (b, j) at key_pad[b*key_pad_sb + j]; non-zero = key j of image b takes
     * no part for ANY query of that image: probability exactly 0, nothing added to lse, out, sv or a bucket gradient;
     * dk = dv = 0 and a zero dlq row at that key, whatever its k / v rows hold.  Queries at padded positions attend
     * to the real keys like every other query.  NULL: no mask.  PRECONDITION: at least one real key per image — an
     * image whose keys are all masked gets non-finite out / lse rows (the reference gives NaN), without a fault.
     * The SAME mask must be given to the backward call. */
    const uint8_t* key_pad;
    int64_t key_pad_sb;
    /* out (fwd: written; bwd: read) and dout: element (b, n, h, :) at ptr[b*osb + n*osn + h*head_dim] resp.
     * ptr[b*dosb + n*dosn + h*head_dim], so that sequence-first (L, N, E) tensors need no copy.  Multiples of 8.
     * osb = osn = 0 (dosb = dosn = 0): contiguous (B, L, H, head_dim) as in the base block. */
    int64_t osb, osn, dosb, dosn;
} cream_irpe_attn2_desc;

/* The argument check of the two calls below alone (backward != 0: of cream_irpe_attn2_bwd): CREAM_OK or the error
 * code the call would return before launching.  Touches no device. */
int cream_irpe_attn2_check(const cream_irpe_attn2_desc* d, int backward);

/* out, lse (and sv) from q, k, v.  One launch.  Reads: q, k, v, tables, id* (query-major), key_pad. */
int cream_irpe_attn2_fwd(const cream_irpe_attn2_desc* d, void* stream);

/* dq, dk, dv and the bucket-gradient rows dlk, dlq from dout (+ out, lse, sv-independent).  Pre-pass (with wq): the
 * (k * scale) Wq rows of all keys into dlq.  Launch A (lanes own queries) reads q, k, v, out, dout, lse, the
 * query-major ids, key_pad and the pre-pass rows; writes delta, dq, dlk and the scratch rows lkg, gg.  Launch B (lanes
 * own keys) reads q, k, v, dout, lse, delta, lkg, gg, the key-major ids (id*_t) and key_pad; writes dk, dv and, last,
 * dlq.  delta, lkg, gg are scratch.  No global atomics: two calls on the same operands give the same bits. */
int cream_irpe_attn2_bwd(const cream_irpe_attn2_desc* d, void* stream);

/* cream_irpe_table_grad for the widths of the calls above: out[b*H+h][a][c] = mul * sum_n X[b,n,h][a] * Y[b,n,h][c],
 * (xa x yc) fp32 per (b, h), xa / yc = the row widths of X / Y, each 32 | 64 | 128 (CREAM_ERR_BAD_ARG otherwise):
 *   d lookup_table_weight(rpe_k) = (scale q)^T dlk  (head_dim x row_width), (rpe_q) = (scale k)^T dlq,
 *   (rpe_v) = sv^T dout  (row_width x head_dim).  Rows of padded keys are zero in dlq; rows n >= L are not read. */
int cream_irpe_table_grad2(float* out, const void* x, int64_t xsb, int64_t xsn, int64_t xsh, int xa, const void* y,
                           int64_t ysb, int64_t ysn, int64_t ysh, int yc, int B, int H, int L, float mul, void* stream);

/* ---- HBM-bound passes of one supernet transformer block ------------------------------------
 * Reference: TransformerEncoderLayer.forward, AutoFormer/model/supernet_transformer.py:251-287
 * (pre-norm block), LayerNormSuper.forward (model/module/layernorm_super.py:26-37), gelu in
 * fp32 (supernet_transformer.py:14-16), DropPath (model/utils.py:68-98).  The residual stream
 * is fp32 (as under the reference's autocast), GEMM operands are bf16.  All matrices are
 * row-major and contiguous with leading dimension = their width.  No atomics anywhere. */

/* y(bf16, M x E) = LayerNorm(x(f32))*gamma + beta over the last dim; mean/rstd (M) saved. */
int cream_ln_fwd(void* y, float* mean, float* rstd, const float* x, const float* gamma,
                 const float* beta, int M, int E, float eps, void* stream);

/* Residual add fused with the following LayerNorm (supernet_transformer.py:266-275: the
 * attention branch's  x = residual + drop_path(x)  and the  ffn_layer_norm  that reads it):
 * xsum(f32) = x(f32) + sample_scale[row / rows_per_sample] * res(bf16)  (scale may be NULL = 1),
 * y(bf16) = LayerNorm(xsum), mean/rstd of xsum saved. */
int cream_add_ln_fwd(float* xsum, void* y, float* mean, float* rstd, const float* x, const void* res,
                     const float* sample_scale, int rows_per_sample, const float* gamma,
                     const float* beta, int M, int E, float eps, void* stream);

/* Number of row slabs ln_bwd reduces over: partial must hold cream_ln_partials()*3*E floats. */
int cream_ln_partials(void);

/* dx(f32) = dres + dLayerNorm(dy(bf16)); if dx_scaled != NULL also writes
 * bf16(dx * sample_scale[row / rows_per_sample]) (sample_scale may be NULL = 1): the gradient
 * entering the previous residual branch with its drop-path scale.  dres may be NULL.
 * partial[p][0][:] / partial[p][1][:] = per-slab sums for dgamma / dbeta; partial[p][2][:] =
 * column sums of the bf16 values written to dx_scaled (= bias gradient of the projection
 * whose output gradient dx_scaled is; zeros when dx_scaled is NULL).  The caller adds the
 * slabs (cream_grad_finalize): fixed order. */
int cream_ln_bwd(float* dx, void* dx_scaled, float* partial, const void* dy, const float* x,
                 const float* mean, const float* rstd, const float* gamma, const float* dres,
                 const float* sample_scale, int rows_per_sample, int M, int E, void* stream);

/* g = gelu(h) / dh = dg * gelu'(h): exact erf GELU evaluated in fp32, bf16 storage; n % 8 == 0 */
int cream_gelu_fwd(void* g, const void* h, int64_t n, void* stream);
int cream_gelu_bwd(void* dh, const void* dg, const void* h, int64_t n, void* stream);

/* out(f32) = x(f32) + sample_scale[i / per_sample] * y(bf16)   (flat index i; scale may be NULL) */
int cream_residual_add(float* out, const float* x, const void* y, const float* sample_scale,
                       int64_t n, int64_t per_sample, void* stream);

/* out(bf16) = sample_scale[i / per_sample] * x(f32) */
int cream_scale_cast(void* out, const float* x, const float* sample_scale, int64_t n,
                     int64_t per_sample, void* stream);

/* Bias gradients: partial[s][c] = sum of a(bf16, M x C)[r][c] over the rows of slab s
 * (cream_colsum_slabs(M) slabs of 512 rows); the caller adds the slabs. */
int cream_colsum_slabs(int M);
int cream_colsum(float* partial, const void* a, int M, int C, void* stream);

/* The same passes with the bias gradient riding along (what autograd's sum-to-size of
 * F.linear's bias produces, Linear_super.py:52-54 / qkv_super.py:49-51), 128-row slabs:
 * partial[s][c] = sum over the rows of slab s of the bf16-ROUNDED values written (so the result
 * equals cream_colsum of the output), cream_colsum128_slabs(M) slabs, C % 8 == 0.
 *   cream_gelu_bwd_colsum    dh(bf16, M x C) = dg * gelu'(h)                    (fc1 bias)
 *   cream_scale_cast_colsum  out(bf16, M x C) = sample_scale[row / rows_per_sample] * x(f32)
 *                                                                                  (fc2 bias)
 *   cream_colsum128          column sums only (qkv bias: dqkv leaves the attention kernels) */
int cream_colsum128_slabs(int M);
int cream_colsum128(float* partial, const void* a, int M, int C, void* stream);
int cream_gelu_bwd_colsum(void* dh, float* partial, const void* dg, const void* h, int M, int C,
                          void* stream);
int cream_scale_cast_colsum(void* out, float* partial, const float* x, const float* sample_scale,
                            int rows_per_sample, int M, int C, void* stream);

/* ---- dense projections of the weight-entangled Linear layers ---------------------------------
 * LinearSuper.forward / qkv_super.forward = F.linear(x, W[:out, :in], b[:out])
 * (AutoFormer/model/module/Linear_super.py:38-54,71-81; qkv_super.py:45-55,72-83), the erf-GELU of
 * the Mlp (supernet_transformer.py:14-16,275-285) and their autograd adjoints, on hand-written MFMA
 * kernels (csrc/gemm_mfma.hpp: direct-to-LDS operand loads, v_mfma_f32_32x32x16_bf16, fused
 * epilogues).  bf16 operands, fp32 accumulation, bf16 results.  The active block of a super weight is
 * read in place: `w` points at element [0][0] of the operand copy, ld = its row stride; N = active
 * out-features, K = active in-features.  Activations are contiguous (row stride = width).
 * N % 8 == K % 8 == ld % 8 == 0, 16-byte aligned pointers.
 *   cream_linear_fwd          out(M x N) = x(M x K) . W(N x K)^T + bias(N)          (bias may be NULL)
 *   cream_linear_fwd_seg      the same with the rows of W in up to 3 segments of `nseg` rows,
 *                             `nseg_stride` elements apart: the de-interleaved [q | k | v] copy of
 *                             the qkv super weight (row n of the product = row n % nseg of segment
 *                             n / nseg) — replaces the torch.cat row gather of qkv_super.py:75
 *   cream_linear_gelu_fwd     with h = bf16(x . W^T + bias): g = gelu(float(h)) and gp = gelu'(float(h)), both
 *                             bf16, in one pass (fc1 + the fp32 gelu of supernet_transformer.py:14-16, on the
 *                             bf16-rounded h exactly as under the reference's autocast; the derivative shares
 *                             Phi and the exponential with the value and is what the backward needs of h);
 *                             gp == NULL: only g is written (a forward without a backward: evaluation sweeps
 *                             of supernet_engine.py:114-160, TinyCLIP's frozen teacher) — half the output bytes
 *   cream_linear_dgrad        dx(M x K) = dy(M x N) . W(N x K); `wt` is the TRANSPOSED copy W^T
 *                             (K rows, N contiguous, row stride ldwt)
 *   cream_linear_dgrad_seg    the same with the contraction index in segments of `kseg` (the
 *                             transposed [q | k | v] copies, `kseg_stride` elements apart; kseg % 64 == 0)
 *   cream_linear_dgrad_mul    dh(M x K) = (dy . W) * factor (bf16, M x K: the saved gelu'(h)) and the column
 *                             sums of dh per 128-row slab: colsum_parts[slab][K] (fc2 dgrad + GELU backward +
 *                             fc1 bias gradient partials, cream_gemm_rows_per_colsum_slab() rows per slab)
 *   cream_linear_wgrad_parts  parts[s](N x K) fp32 = dy_s^T x_s over S slices of the M rows (slices of
 *                             whole 64-row steps, as even as possible; added by cream_grad_finalize);
 *                             bias_parts[s](N) = column sums of dy_s — the bias gradient rides on the
 *                             same kernel (NULL: not wanted).  cream_linear_wgrad_splits gives the S
 *                             this library uses for a problem (~1 workgroup per CU, at most 16). */
int cream_gemm_rows_per_colsum_slab(void);

/* Tile choice of the NT products (Linear_super.py:38-54, qkv_super.py:45-55 and their dgrads): where the 256 x 256 macro
 * tile (8 waves, 128 KB of LDS, one persistent workgroup per CU) replaces the 128-wide tiles (two to three workgroups per CU).
 * 0 = nowhere; 1 = wide outputs (N >= 960: qkv / fc1 forward, fc2 dgrad); 2 = long contractions (K >= 1152: fc2 forward,
 * fc1 dgrad, qkv dgrad at embed dim >= 384) — the default: 6-14 % faster there with cold operands; 3 = K >= 960.
 * on < 0 only queries; returns the previous setting; the initial one comes from CREAM_GEMM_NT256 in the environment.
 * Results are identical in every mode (same products, same epilogues). */
int cream_gemm_nt256(int on);
/* Schedule of the NT products (same reference functions): the counted-vmcnt, phase-interleaved kernel of csrc/gemm_nt8.hpp
 * (256 x 256 tiles, 8 waves in two staggered rows, a whole K-tile of LDS-DMA requests in flight across every barrier, K-tile
 * stream continuous over output tiles, barrier-free per-wave epilogue).  0 = never (the kernels above), 1 = wherever its
 * limits allow (31-bit element offsets), 2 = plain and bias products everywhere, the GELU / x gelu' epilogues only on long
 * contractions (K >= 1024); 3 = plain and bias products whose 256-wide column tiles carry at most 1/8 padding; 4 = the forward
 * products (bias epilogue) under the same padding bound — the DEFAULT (no weight-gradient stream runs beside the forward) —
 * plus every product whose output AND contraction are at least 640 wide (DeiT-base / CLIP ViT-B blocks; no AutoFormer shape).
 * mode < 0 only queries; returns the previous setting; the initial one comes from CREAM_GEMM_NT8 in the environment.
 * Forward, bias, bias + GELU results are identical to the other kernels'.  cream_linear_dgrad_mul: when this kernel serves it
 * (modes 1 and 2) dy . W is rounded to bf16 before the multiplication by gelu' (as the reference's two operators do); the
 * two-stage kernels (modes 0, 3, 4 — the default) multiply the fp32 accumulator and round once — the results differ by at
 * most one bf16 rounding of the product. */
/* Round 6: 256 x (E / 2) tiles (column tiles that divide N) for the plain / bias products whose output is 320 / 384 / 448 wide
 * (csrc/gemm_mfma.hip: launch_nt_half).  1 = on, 0 = off, < 0 queries; returns the previous value; initial: CREAM_GEMM_NTHALF. */
int cream_gemm_nthalf(int on);
/* A 256 x 224 tile on v_mfma_f32_16x16x32_bf16 (csrc/gemm_nt224.hpp, launch_nt224 in csrc/gemm_mfma.hip) for the plain / bias
 * products whose output is 448 wide at M >= 1024 (proj, fc2 and the fc1 / qkv / proj input gradients at embed dim 448; the proj
 * input gradient at 7 heads) and for cream_linear_fwd_seg with N = 1344 in
 * segments of 448 (qkv forward at 7 heads).  1 = on (default), 0 = off, < 0 queries; returns the previous value; initial:
 * CREAM_GEMM_NT224.
 * This instruction adds 32 contraction elements per issue, the other tiles 16: on general operands a routed product may differ
 * from the switch-off result in the last bf16 place.  No workspace layout depends on the switch. */
int cream_gemm_nt224(int on);
/* Launches of that tile by this process so far (routed calls and cream_linear_nt224): a test reads it around a call to see
 * which kernel the call reached. */
int64_t cream_gemm_nt224_launches(void);
/* The same tile on any problem, whatever the switches say (tests, probes): out(M x N) = x(M x K) . W(N x K)^T + bias (bias may be
 * NULL: plain store).  nseg > 0: rows of W in segments as cream_linear_fwd_seg; kseg > 0: the contraction in segments as
 * cream_linear_dgrad_seg (K % kseg == 0, kseg % 64 == 0); 0 = one segment.  M arbitrary, N % 8 == K % 8 == ldw % 8 == 0. */
int cream_linear_nt224(void* out, const void* x, const void* w, const void* bias, int M, int N, int K, int64_t ldw, int nseg,
                       int64_t nseg_stride, int kseg, int64_t kseg_stride, void* stream);
/* A full-row 256 x E tile (csrc/gemm_ntrow.hpp, launch_ntrow in csrc/gemm_mfma.hip) for the plain-store products (the input
 * gradients cream_linear_dgrad / cream_linear_dgrad_seg) whose output is exactly 384 or 320 wide at M >= 1024: one persistent
 * workgroup per CU walks 256-row panels.  1 = on (default), 0 = off, < 0 queries; returns the previous value; initial:
 * CREAM_GEMM_NTROW.  Results are bit-identical to the switch-off route.  No workspace layout depends on the switch. */
int cream_gemm_ntrow(int on);
/* Launches of that tile by this process so far: a test reads it around a call to see which kernel the call reached. */
int64_t cream_gemm_ntrow_launches(void);
/* The same tile whatever the switch says (tests, probes): out(M x N, row stride ldo) = x(M x K, row stride ldx) . W(N x K)^T, plain
 * store.  N must be 384 or 320; kseg > 0: the contraction in segments as cream_linear_dgrad_seg (K % kseg == 0, kseg % 64 == 0);
 * 0 = one segment.  M arbitrary, K % 8 == ldw % 8 == ldo % 8 == ldx % 8 == 0. */
int cream_linear_ntrow(void* out, int64_t ldo, const void* x, int64_t ldx, const void* w, int M, int N, int K, int64_t ldw, int kseg,
                       int64_t kseg_stride, void* stream);
int cream_gemm_nt8(int mode);
/* Round 6: the two-stage NT kernels with their tile epilogue taken off the memory counters (csrc/gemm_mfma.hpp, "OPT"):
 * bit 0 = LDS-DMA as asm, LDS-only epilogue barriers, side inputs (bias, the x gelu' factor rows) requested under the first
 * K-step, counted vmcnt for the first K-step behind an epilogue — on the 128-wide tiles of the forward products (bias, bias +
 * GELU); bit 3 (8) = also on the backward's (plain store, x gelu'); bit 2 (4) = also on the 256-wide macro tiles; bit 1 = gelu(h) /
 * gelu'(h) of cream_linear_gelu_fwd from a 16 KB LDS table over the bf16 values of h (filled by the same function the direct
 * path evaluates).  Default 3, < 0 queries; returns the previous value; initial: CREAM_GEMM_NTOPT.  Results are bit-identical in every mode
 * (tests/test_block_gpu.py::test_nt_epilogue_variants_are_bit_identical; the table exhaustively over all bf16 h, with the one
 * exception |h| < 2^-125, where gelu(h) differs by less than 1.2e-38). */
int cream_gemm_ntopt(int mode);
/* The second half of a two-workgroups-per-CU NT grid starts n x 64 clocks late (A/B switch; default 0); < 0 queries. */
int cream_gemm_stagger(int n);
int cream_linear_fwd(void* out, const void* x, const void* w, const void* bias, int M, int N, int K,
                     int64_t ldw, void* stream);
int cream_linear_fwd_seg(void* out, const void* x, const void* w, const void* bias, int M, int N, int K,
                         int64_t ldw, int nseg, int64_t nseg_stride, void* stream);
int cream_linear_gelu_fwd(void* gp, void* g, const void* x, const void* w, const void* bias, int M, int N,
                          int K, int64_t ldw, void* stream);
/* The same with N rounded up to a multiple of 8: outputs of columns n >= Nvalid are written as zeros. */
int cream_linear_gelu_fwd_pad(void* gp, void* g, const void* x, const void* w, const void* bias, int M, int N, int Nvalid,
                              int K, int64_t ldw, void* stream);
int cream_linear_dgrad(void* dx, const void* dy, const void* wt, int M, int N, int K, int64_t ldwt,
                       void* stream);
int cream_linear_dgrad_seg(void* dx, const void* dy, const void* wt, int M, int N, int K, int64_t ldwt,
                           int kseg, int64_t kseg_stride, void* stream);
int cream_linear_dgrad_mul(void* dh, float* colsum_parts, const void* dy, const void* wt, const void* factor,
                             int M, int N, int K, int64_t ldwt, void* stream);
int cream_linear_wgrad_splits(int M, int N, int K);
int cream_linear_wgrad_parts(float* parts, float* bias_parts, const void* dy, const void* x, int M, int N,
                             int K, int S, void* stream);
/* The same with the partial tiles written as bf16 [S][N][K] (half the partial traffic: 113 instead of 226 MB per
 * transformer block through HBM, written here and read by cream_grad_finalize with src_bf16 = 1).  Every split's sum over
 * its ~M / S tokens is rounded to bf16 once — what torch.autocast's backward does to the WHOLE gradient of the bf16 weight
 * copy (Linear_super.py:71-81 under autocast); the bias partials stay fp32. */
int cream_linear_wgrad_parts_bf16(void* parts_bf16, float* bias_parts, const void* dy, const void* x, int M, int N,
                                  int K, int S, void* stream);
/* The split count for a weight gradient with bf16 partial tiles (Linear_super.py:71-81, qkv_super.py:72-83 backward).
 * cream_linear_wgrad_parts_bf16 called with THIS split count runs the macro-tile kernel of csrc/gemm_tn8.hpp (256 x 256 tile on
 * the phase-interleaved loop, one 8-wave workgroup per CU, token slices for half the CUs — the weight gradients share the chip
 * with the main chain and every slice is another partial tile through HBM); bias partials ride along.  With any other S, or with
 * fp32 partials (cream_linear_wgrad_parts), the 128 x 128 kernel runs.  Same partial-tile layout and rounding either way.
 * cream_gemm_tn8(0 | 1 | 2): never / problems of at least six 256 x 256 tiles / every problem (default); < 0 queries.
 * Changing it changes cream_linear_wgrad_splits_bf16 and with it the backward workspace layout (cream_block_layout_epoch). */
int cream_linear_wgrad_splits_bf16(int M, int N, int K);
int cream_gemm_tn8(int mode);

/* ---- parameter update + operand copies ------------------------------------------------------
 * torch.optim.AdamW as created by timm's create_optimizer (AutoFormer/supernet_train.py:294-296;
 * decoupled weight decay, bias-corrected moments) over EVERY tensor of the model in one launch, which
 * also writes the bf16 operand copies the GEMM kernels read: `mir` = the tensor as (rows x cols) bf16
 * with row stride ld_mir, `mir_t` = its transpose (cols x rows, row stride ld_mir_t) or NULL;
 * deinterleave != 0 (the qkv super weight, qkv_super.py:75): row 3 i + j of the tensor is row i of
 * part j — parts seg_stride (seg_stride_t) elements apart in the copies.  g == NULL or update == 0:
 * copies only (initialisation, checkpoint load).  The job table and the prefix sums of
 * cream_param_job_tiles(rows, cols) over the jobs (njobs + 1 entries) live in DEVICE memory. */
typedef struct cream_param_job {
    float* p;              /* fp32 master tensor viewed as (rows x cols), row stride ld          */
    const float* g;        /* gradient (same layout) or NULL                                    */
    float *m, *v;          /* exp_avg, exp_avg_sq                                               */
    void *mir, *mir_t;     /* bf16 copies or NULL                                               */
    int64_t ld, ld_mir, ld_mir_t, seg_stride, seg_stride_t;
    int32_t rows, cols, deinterleave;
    float weight_decay;
} cream_param_job;
int cream_param_job_tiles(int rows, int cols);
int cream_adamw_step(const cream_param_job* jobs_dev, const int32_t* first_tile_dev, int njobs, int total_tiles,
                     int update, double lr, double beta1, double beta2, double eps, int64_t step, void* stream);

/* Global-norm gradient clipping (torch.nn.utils.clip_grad_norm_, norm_type 2) over the same job table, without a host
 * synchronisation and without a second pass over the gradients:
 *     out[0] = sqrt(sum over every job with g != NULL of g[r, c]^2),   r < rows, c < cols (columns cols..ld are never read)
 *     out[1] = min(1, max_norm / (out[0] + 1e-6))                      (torch.nn.utils.clip_grads_with_norm_)
 * max_norm > 0; +inf gives the norm alone (out[1] = 1).  A non-finite norm propagates as in torch (inf -> 0, NaN -> NaN).
 * The summation order is fixed — fp32 over a thread's at most 24 elements, fp64 over the workgroup into partials_dev[tile],
 * fp64 over the partials in index order — so the result is bit-reproducible and independent of scheduling; every entry of
 * partials_dev (total_tiles doubles) is rewritten by every call.  With no tiles out = {0, 1}.
 * cream_adamw_step_clipped is cream_adamw_step with every gradient value multiplied by *coef_dev (one fp32 multiply) as it
 * is loaded: the gradient tensors themselves are NOT modified (torch's clip_grad_norm_ scales them in place).
 * cream_grad_scale does scale them in place (g *= *coef_dev), for an optimizer that is not cream_adamw_step; with
 * *coef_dev == 1 nothing is read or written.
 * cream_grad_clip_coef and cream_grad_scale read only g, rows, cols and ld of a job: p (and m, v, the copies) may be NULL. */
int cream_grad_clip_coef(const cream_param_job* jobs_dev, const int32_t* first_tile_dev, int njobs, int total_tiles,
                         double max_norm, double* partials_dev, float* out_dev, void* stream);
int cream_adamw_step_clipped(const cream_param_job* jobs_dev, const int32_t* first_tile_dev, int njobs, int total_tiles,
                             int update, double lr, double beta1, double beta2, double eps, int64_t step,
                             const float* coef_dev, void* stream);
int cream_grad_scale(const cream_param_job* jobs_dev, const int32_t* first_tile_dev, int njobs, int total_tiles,
                     const float* coef_dev, void* stream);

/* cream_adamw_step with one learning rate PER PARAMETER GROUP — the layer-wise learning-rate decay of TinyViT's fine-tune
 * recipes (TinyViT/optimizer.py:13-37 with tinyvit_utils.divide_param_groups_by_lr_scale: one torch.optim.AdamW group per
 * lr_scale and weight-decay class, whose `lr` LRSchedulerWrapper rewrites after every scheduler call).
 *     group_of_job_dev   njobs int32 in DEVICE memory: the group of every job of the table
 *     lr_of_group        ngroups doubles in HOST memory, 1 <= ngroups <= CREAM_ADAMW_MAX_GROUPS; rounded to fp32 and passed
 *                        to the kernel by value (256 bytes of kernel arguments), so a schedule that changes them every step
 *                        costs no device buffer, no copy and no synchronisation
 * A job's workgroups take lr_of_group[group_of_job_dev[job]]; a stored index outside [0, ngroups) is CLAMPED to the last
 * group (never read past the argument).  Everything else is cream_adamw_step's: the per-element arithmetic of a job is the
 * instruction sequence of the ungrouped kernel run with that job's rate, weight_decay stays per job, the copies, g == NULL
 * and update == 0 behave alike.  beta1, beta2, eps and the step counter (bias correction) stay COMMON to all groups.
 * coef_dev NULL: unclipped; else cream_adamw_step_clipped's coefficient (cream_grad_clip_coef's norm is global over all
 * groups, as clip_grad_norm_ over model.parameters() is).
 * CREAM_ERR_BAD_ARG without launching: ngroups outside 1..CREAM_ADAMW_MAX_GROUPS, a NULL lr_of_group, a NULL
 * group_of_job_dev with njobs > 0, update with step < 1, NULL tables; njobs == 0 or total_tiles == 0 is a no-op. */
#define CREAM_ADAMW_MAX_GROUPS 64
int cream_adamw_step_groups(const cream_param_job* jobs_dev, const int32_t* first_tile_dev, int njobs, int total_tiles,
                            int update, const int32_t* group_of_job_dev, const double* lr_of_group, int ngroups,
                            double beta1, double beta2, double eps, int64_t step, const float* coef_dev, void* stream);

/* Gradient finalisation for the weight-entangled parameters: every tensor of a block gets
 *     dst[map(r)*ld + c] += sum_p src[p*pstride + r*cols + c]          r < rows, c < cols
 * in ONE launch — dst is the ACTIVE SLICE W[:out, :in] of the fp32 super-weight gradient
 * (ld = super width; what autograd's backward of the slicing in Linear_super.py:71-81 and
 * qkv_super.py:72-83 accumulates), src are partial sums produced upstream (split-K weight
 * gradient GEMMs, per-slab column sums, per-(batch, head) table gradients).  interleave = Q > 0:
 * the rows of src are grouped [q | k | v] (Q each) and row r goes to super row
 * 3*(r % Q) + r / Q — the adjoint of qkv_super's row gather (qkv_super.py:75).  Parts are
 * added in a fixed tree: bit-reproducible.  cols, ld, pstride % 4 == 0. */
typedef struct cream_grad_job {
    float* dst;
    const void* src;
    int64_t ld;
    int64_t pstride;       /* elements between consecutive parts */
    int32_t nparts, rows, cols;
    int32_t interleave;
    int32_t src_bf16;      /* partials are bf16 (1) or fp32 (0) */
    int32_t overwrite;     /* 0: dst += sum of the parts; 1: dst = sum (a gradient that did not exist yet: the caller allocates it
                              uninitialised instead of zero-filling it; the job must cover all of dst) */
} cream_grad_job;
#define CREAM_MAX_GRAD_JOBS 24
int cream_grad_finalize(const cream_grad_job* jobs, int njobs, void* stream);

/* ---- TinyCLIP's pruning masks folded into the operands (csrc/l0_mask.hip) ------------------------------------------------
 * TinyCLIP/src/open_clip/l0module.py; model.py:40-68 (masked LayerNorm), :131-136 and :273-282 (hidden_z / heads_z /
 * intermediate_z on c_proj and out_proj).  With zh (D), zd (H) expanded to 64 columns per head, zi (F):
 *     Wo' = diag(zh) Wo diag(e(zd)),  bo' = zh * bo,  W2' = diag(zh) W2 diag(zi),  b2' = zh * b2
 * the masked block is the dense block on these operands with the masked LayerNorm in place of ln_1 / ln_2.
 *
 * Masked LayerNorm: the contracts of cream_ln_fwd / cream_add_ln_fwd / cream_ln_bwd with a mask z (E floats, 16-byte aligned):
 * column c is KEPT iff z[c] != 0, and n_keep is the number of kept columns as the caller counted it (1 <= n_keep <= E;
 * n_keep <= 0 returns CREAM_ERR_BAD_ARG and launches nothing).  Mean and variance are over the kept columns only, divisor
 * n_keep — the dropped columns are selected away, not multiplied: whatever they hold, finite or not, never enters a sum.
 * y is exactly 0 in the dropped columns (n_keep == 1: variance 0, y = beta in the kept column).  xsum is x + scale * res in
 * EVERY column.  Backward: dy of a dropped column is discarded, the LayerNorm's contribution to dx and the dgamma / dbeta
 * partials are exactly 0 there, dres passes through in every column, dx_scaled and the third partial row cover every
 * column as in cream_ln_bwd.  No gradient reaches z (the reference selects by torch.where(hidden_z != 0)). */
int cream_ln_fwd_masked(void* y, float* mean, float* rstd, const float* x, const float* gamma, const float* beta,
                        const float* z, int n_keep, int M, int E, float eps, void* stream);
int cream_add_ln_fwd_masked(float* xsum, void* y, float* mean, float* rstd, const float* x, const void* res,
                            const float* sample_scale, int rows_per_sample, const float* gamma, const float* beta,
                            const float* z, int n_keep, int M, int E, float eps, void* stream);
int cream_ln_bwd_masked(float* dx, void* dx_scaled, float* partial, const void* dy, const float* x, const float* mean,
                        const float* rstd, const float* gamma, const float* z, int n_keep, const float* dres,
                        const float* sample_scale, int rows_per_sample, int M, int E, void* stream);

/* Masked operand pack, several tensors per launch (the job table is HOST memory, copied into the launch):
 *     mir[i * ld_mir + k]     = bf16((w[i * ld + k] * r[i]) * c[k / c_group])        i < rows, k < cols
 *     mir_t[k * ld_mir_t + i] = the same value
 * the products in fp32 in this order, rounded once to nearest-even; r == NULL / c == NULL: that factor is absent.  c_group is
 * 1 (a factor per column) or 64 (a factor per head of 64 columns).  mir or mir_t may be NULL (not both).  A bias b (n) with
 * its mask is the job rows = 1, cols = n, c = the mask.  cols, ld, ld_mir % 4 == 0; with mir_t also rows, ld_mir_t % 4 == 0;
 * w 16-byte, the copies 8-byte aligned. */
typedef struct cream_mask_pack_job {
    const float* w;
    const float* r;        /* rows entries or NULL                       */
    const float* c;        /* cols / c_group entries or NULL             */
    void *mir, *mir_t;     /* bf16 (rows x cols) / (cols x rows) or NULL */
    int64_t ld, ld_mir, ld_mir_t;
    int32_t rows, cols, c_group, reserved;
} cream_mask_pack_job;
#define CREAM_MAX_MASK_JOBS 16
int cream_mask_pack_check(const cream_mask_pack_job* jobs, int njobs);
int cream_mask_pack(const cream_mask_pack_job* jobs, int njobs, void* stream);

/* Masked gradient finalisation: src holds the partial sums of the gradient of an EFFECTIVE operand W' = diag(r) W diag(c)
 * (layout, src_bf16 and overwrite as in cream_grad_job; no interleave).  With G = sum_p src[p] in the summation tree of
 * cream_grad_finalize:
 *     dst[i * ld + k] (+)= (r[i] * c[k / c_group]) * G[i, k]                          (the gradient of W)
 *     dr_out[i]       (+)= sum_k (G[i, k] * w[i, k]) * c[k / c_group]                 (the gradient of r; dr_accumulate)
 *     dc_out[g]       (+)= sum_{k in group g} sum_i (G[i, k] * w[i, k]) * r[i]        (the gradient of c; dc_accumulate)
 * r / c == NULL: that factor is 1; dr_out / dc_out == NULL: not computed.  A bias is the job rows = 1, cols = n, c = its mask,
 * dc_out = the mask's gradient.  The matrix is walked in fixed 16 x 64 tiles; a tile's row and column sums go to ws
 * (cream_mask_grad_ws_floats(rows, cols) floats per job, required with dr_out or dc_out) and a second launch adds them in
 * ascending tile order: every result is bit-reproducible and independent of the grid (cream_cu_reserve).  Within one call no
 * two jobs may share dst, dr_out, dc_out or ws (CREAM_ERR_BAD_ARG): every output has one writer.  Host job table. */
typedef struct cream_mask_grad_job {
    float* dst;
    const void* src;
    const float* w;        /* the fp32 master tensor, row stride ld_w */
    const float* r;
    const float* c;
    float* dr_out;
    float* dc_out;
    float* ws;
    int64_t ld, pstride, ld_w;
    int32_t nparts, rows, cols, c_group, src_bf16, overwrite, dr_accumulate, dc_accumulate;
} cream_mask_grad_job;
int64_t cream_mask_grad_ws_floats(int rows, int cols);
int cream_mask_grad_check(const cream_mask_grad_job* jobs, int njobs);
int cream_mask_grad_finalize(const cream_mask_grad_job* jobs, int njobs, void* stream);

/* ---- pruned TinyCLIP towers on zero-padded operands (csrc/pruned_ops.hip) ------------------------------------------------
 * A tower cut by prune() (TinyCLIP/src/open_clip/model.py:139-205, :317-339) has a stream of d = len(kept hidden) columns and
 * per-layer MLP widths F_l, any integers.  It runs as the dense node on operands padded with zeros to the GEMM granularity
 * (Dp, Fp_l: multiples of 8); parameters and gradients keep their compact shapes.
 *
 * Compact gradient finalisation: split-K partials laid out on the PADDED shape, added into a COMPACT fp32 gradient
 *     dst[r * ld_dst + c] (+)= sum_p src[p * pstride + r * ld_src + c]              r < rows, c < cols
 * rows, cols, ld_dst >= cols: any positive integers; dst 4-byte aligned only.  ld_src >= cols; src 16-byte aligned; ld_src and
 * pstride multiples of 8 (bf16 partials) or 4 (fp32 partials).  The source is read in 16-byte chunks, so columns cols .. ld_src
 * of a source row may be read — their values never reach dst —; nothing of dst outside rows x cols is read or written.  Per
 * element the sum is the tree of cream_grad_finalize (csrc/grad_tree.hpp): the result equals, bit for bit, cream_grad_finalize
 * into a (rows x ld_src) buffer followed by a slice.  Host job table, one launch; two jobs never share dst. */
typedef struct cream_grad_compact_job {
    float* dst;
    const void* src;
    int64_t ld_dst, ld_src;
    int64_t pstride;       /* elements between consecutive parts */
    int32_t nparts, rows, cols;
    int32_t src_bf16;      /* partials are bf16 (1) or fp32 (0) */
    int32_t overwrite;     /* as in cream_grad_job */
    int32_t reserved;
} cream_grad_compact_job;
#define CREAM_MAX_COMPACT_JOBS 24
int cream_grad_finalize_compact_check(const cream_grad_compact_job* jobs, int njobs);
int cream_grad_finalize_compact(const cream_grad_compact_job* jobs, int njobs, void* stream);

/* Rows between the compact and the padded layout, one launch each:
 *     cream_pad_cols:    out (M x Dp) fp32 = in (M x d, contiguous rows, in_dtype CREAM_F32 or CREAM_BF16) in columns < d, 0 in d .. Dp
 *     cream_unpad_cols:  out (M x d, contiguous rows, out_dtype CREAM_F32 or CREAM_BF16, round to nearest even) = in (M x Dp) fp32
 * 1 <= d <= Dp, Dp % 4 == 0; the padded side 16-byte aligned, the compact side aligned to its element only.  M == 0: no-op. */
int cream_pad_cols(float* out, const void* in, int in_dtype, int M, int d, int Dp, void* stream);
int cream_unpad_cols(void* out, int out_dtype, const float* in, int M, int d, int Dp, void* stream);

/* ---- the uint8 -> normalised float input transform of a batch, on the device (csrc/image_transform.hip) -----------------
 * AutoFormer/lib/datasets.py:189-220 (`build_transform`): eval = Resize(int(256 / 224 * input_size), bicubic) -> CenterCrop ->
 * ToTensor -> Normalize; train = timm's RandomResizedCropAndInterpolation(bicubic) -> RandomHorizontalFlip -> [RandAugment: host
 * side] -> ToTensor -> Normalize.  On the reference's PIL images every resize is Pillow's Image.resize(size, BICUBIC); the kernels
 * restate that 8-bit algorithm (libImaging/Resample.c, 22-bit fixed-point coefficients from doubles, horizontal pass then vertical
 * pass with a uint8 intermediate) integer for integer, then torchvision's x / 255 and (x - mean) / std in float32: byte-exact
 * against Pillow, bit-exact against torch's CPU ops (tests/test_image_transform_gpu.py).
 * One image: the decoded frame (HWC uint8 RGB at pixels + offset, row_stride bytes per row), the box F.crop takes, the size F.resize
 * gives the crop, the (win_top, win_left) + (out_h, out_w) window of the resized image that becomes the output (CenterCrop; (0, 0) with
 * resized == out for the training crop) and the mirror flag of RandomHorizontalFlip.
 * cream_image_batch_plan (host only, no device work) validates the B descriptors, fills row0 / nrows (the box rows the window's
 * vertical pass reads) and tmp_off, and returns the workspace size in bytes (>= 0) or an error code (< 0): CREAM_ERR_TOO_LARGE when
 * a crop is wider than 4776 pixels or shrinks by more than (40960 / (4 out_w) - 1) / 4 (x 11 at out_w = 224).
 * cream_image_batch_transform takes the planned descriptors twice — the host array (validated again, sizes the grids) and a copy
 * of it in device memory (the caller uploads it as it likes: one async copy from pinned memory) — and enqueues three launches (coefficient tables, horizontal pass, vertical pass + float tail) on
 * `stream`: out (B, 3, out_h, out_w) fp32.  pixels: 4-byte aligned, pixels_bytes a multiple of 4 (rows are staged with aligned
 * 4-byte loads); out, workspace: 16-byte aligned; out_w % 4 == 0, out_w <= 1024. */
typedef struct cream_image_desc {
    int64_t offset;                                 /* byte offset of the frame in `pixels` */
    int32_t height, width, row_stride;              /* decoded frame; row_stride >= 3 * width bytes */
    int32_t box_top, box_left, box_h, box_w;        /* F.crop */
    int32_t resized_h, resized_w;                   /* F.resize of the crop */
    int32_t win_top, win_left;                      /* window of the resized image */
    int32_t flip;                                   /* != 0: mirrored */
    int32_t row0, nrows;                            /* filled by cream_image_batch_plan */
    int64_t tmp_off;                                /* filled by cream_image_batch_plan */
    /* RandomErasing of the training recipe (timm, mode 'pixel': lib/datasets.py:199-201 re_prob / re_mode / re_count), applied to
     * the NORMALISED output: elements [:, erase_top : + erase_h, erase_left : + erase_w] become standard-normal noise, a pure
     * function of (erase_seed, channel, row, column) (a counter-based hash through Box-Muller); erase_h == 0: no erasing.  The box
     * is drawn on the host (autoformer/data.py: random_erasing_params, timm's order of draws); the noise stream is this library's
     * own (no two implementations share one). */
    int32_t erase_top, erase_left, erase_h, erase_w;
    uint32_t erase_seed;
    int32_t reserved;
} cream_image_desc;
int64_t cream_image_batch_plan(cream_image_desc* descs, int B, int out_h, int out_w);
int cream_image_batch_transform(float* out, const uint8_t* pixels, int64_t pixels_bytes, const cream_image_desc* descs,
                                const cream_image_desc* descs_dev, int B, int out_h, int out_w, const float* mean,
                                const float* stdev, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- batch-mode Mixup / CutMix + smoothed soft targets, one launch (csrc/mixup.hip) -----------------
 * `samples, targets = mixup_fn(samples, targets)` of the step body (AutoFormer/supernet_engine.py:52-53; timm.data.Mixup as
 * constructed at supernet_train.py:245-251: mode 'batch' — third-party, not vendored, restated; parity unpinned by the reference,
 * pinned against the host restatement cream_amd/autoformer/data.py).  In place on x (B, Cimg, H, W) fp32, B even, W % 4 == 0:
 *   use_cutmix == 0:  x_b <- lam x_b + (1 - lam) x_{B-1-b}
 *   use_cutmix != 0:  x_b[:, yl:yh, xl:xh] <- x_{B-1-b}[:, yl:yh, xl:xh]   (the caller passes lam corrected for the clipped box)
 *   lam == 1: images untouched.
 * y (B, num_classes) fp32 <- lam onehot_s(target_b) + (1 - lam) onehot_s(target_{B-1-b}), onehot_s = label_smoothing / C off,
 * 1 - label_smoothing + label_smoothing / C on; target (B) int64 class indices.  lambda and the box are drawn by the caller
 * (numpy's global RNG in timm's order: data.Mixup). */
int cream_mixup_cutmix(float* x, float* y, const int64_t* target, int B, int Cimg, int H, int W, int num_classes, float lam,
                       int use_cutmix, int yl, int yh, int xl, int xh, float label_smoothing, void* stream);

/* ---- soft-target cross entropy (loss rows + logit gradient in one launch) --------------------------
 * criterion(outputs, targets) of the step body (AutoFormer/supernet_engine.py:60-66) with timm's
 * SoftTargetCrossEntropy (third-party, not vendored: restated from its published definition —
 * loss = mean_b sum_c -t[b,c] log_softmax(x[b,:])[c]; parity unpinned, as for the framework formulation it replaces):
 *   loss_rows[b] = sum_c t[b,c] (logsumexp(x[b,:]) - x[b,c])                  (the caller takes the mean)
 *   dlogits[b,c] = (softmax(x[b,:])[c] * sum_c t[b,c] - t[b,c]) * grad_scale   f32 (grad_scale = 1 / B for the mean)
 * logits (B x C) bf16 or f32 (logits_dtype), target (B x C) f32, C <= 2048; softmax statistics in fp32. */
int cream_soft_ce(float* loss_rows, float* dlogits, const void* logits, const float* target, int B, int C, int logits_dtype,
                  float grad_scale, void* stream);

/* ---- TinyViT fast distillation: sparse teacher records (csrc/sparse_distill.hip) ------------------
 * cream_sparse_ce: the loss of TinyViT/main.py:321-330 — the dense teacher rebuilt from a top-k record, then the
 * soft-target cross entropy documented at cream_soft_ce — from the SPARSE record, one launch, no B x C target in memory.
 * Per row b, with index (B x k) int16 and value (B x k) fp16 (the record's fields), 1 <= k <= 128, k < C <= 32768:
 *   minor        = (1 - sum_j float(value[b,j])) / (C - k)
 *   t[b,c]       = value[b,j] at c = index[b,j], minor elsewhere
 *   loss_rows[b] = sum_c t[b,c] (logsumexp(x[b,:]) - x[b,c])                  (the caller takes the mean)
 *   dlogits[b,c] = (softmax(x[b,:])[c] * sum_c t[b,c] - t[b,c]) * grad_scale   f32, every element stored exactly once
 * logits (B x C) bf16 or f32 (logits_dtype), rows contiguous (a row of odd length starts at the element's own alignment,
 * which is all the kernel assumes); softmax statistics in fp32; the terms logsumexp - x[c] are summed as terms.
 * Indices within a row are distinct by contract (top-k output).  An index outside [0, C) is never dereferenced: its value
 * counts in `minor` and nowhere else (the host codec rejects such records).
 * Returns CREAM_ERR_TOO_LARGE for k > 128 or C > 32768, CREAM_ERR_BAD_ARG for k >= C, k < 1, a null or misaligned pointer,
 * CREAM_ERR_BAD_DTYPE for other logits types — without launching.
 *
 * cream_softmax_topk_records: the writer side (TinyViT/save_logits.py:135-158): softmax, top-k largest first, straight into
 * the record layout.  records (B x (4 + 4k)) bytes, 4-byte aligned: int32 seed, k int16 indices, k fp16 values.
 * logits (B x C) bf16 or f32, seeds (B) int32, 1 <= k <= 128, k <= C <= 32768.  The ORDER is defined on the logits (softmax is
 * monotone, logits compare exactly): larger logit first, equal logits by ascending class index — stricter than
 * torch.topk, which leaves ties open, and equal to it wherever the fp32 probabilities are distinct.  Values are the fp32
 * softmax rounded to nearest-even fp16; subnormal results are kept.  Error codes as above (k > C is CREAM_ERR_BAD_ARG). */
int cream_sparse_ce(float* loss_rows, float* dlogits, const void* logits, const int16_t* index, const void* value, int B, int C,
                    int k, int logits_dtype, float grad_scale, void* stream);
int cream_softmax_topk_records(void* records, const void* logits, const int32_t* seeds, int B, int C, int k, int logits_dtype,
                               void* stream);

/* ---- fp32-I/O instantiations (parity mode) -------------------------------------------------------
 * The same operators with fp32 tensors on both sides, for the "within 1e-3 of the reference PyTorch-CPU
 * forward / backward" bar: exact-fp32 matrix-core products (v_mfma_f32_32x32x2_f32; gfx950 has no TF32)
 * and the fp32 instantiation of the LayerNorm kernels.
 *
 * cream_linear_f32_fwd   y (M x N) = x (M x K, row stride ldx) . W[wmap(n), :K]^T + bias[:N]
 *                        = LinearSuper.forward / qkv_super.forward (Linear_super.py:38-54, :71-81; qkv_super.py:72-83)
 * cream_linear_f32_dgrad dx (M x K) = dy (M x N) . W[wmap(n), :K]
 * cream_linear_f32_wgrad dW[wmap(n), :K] = dy^T . x  (rows of dw, stride lddw; other rows untouched);
 *                        dbias (N) = column sums of dy in ascending row order, or NULL
 * wmap(r) = (r % seg) * step + r / seg for seg > 0 (qkv super weight: seg = Q, step = 3 — rows 3 i + j,
 * qkv_super.py:75), identity for seg == 0.  w: fp32 super weight, row stride ldw.
 * cream_ln_f32_fwd / _bwd = LayerNormSuper.forward (layernorm_super.py:33-37) and its autograd backward:
 * partial (cream_ln_partials() x 3 x E): planes 0 / 1 = per-slab dgamma / dbeta sums (plane 2 zero). */
int cream_linear_f32_fwd(float* y, const float* x, const float* w, const float* bias, int M, int N, int K, int64_t ldx,
                         int64_t ldw, int seg, int step, void* stream);
int cream_linear_f32_dgrad(float* dx, const float* dy, const float* w, int M, int N, int K, int64_t ldw, int seg, int step,
                           void* stream);
int cream_linear_f32_wgrad(float* dw, float* dbias, const float* dy, const float* x, int M, int N, int K, int64_t ldx,
                           int64_t lddw, int seg, int step, void* stream);
/* cream_bmm_f32  C_z (M x N) = A_z (M x K) . B_z (K x N) for the nb0 x nb1 batch items z = (z0, z1): the attention
 *   products of the iRPE parity mode on the same exact-fp32 matrix-core kernel — q k^T and P v of RPEAttention.forward
 *   (iRPE/DeiT-with-iRPE/rpe_vision_transformer.py:76, :88), the lookup products of irpe.py:641-644 / :683-687 and their
 *   autograd products — instead of the framework's batched matmul (the vendor library).
 *   *_strides[4] = {row, column, z0, z1} ELEMENT strides of each operand (rows of A = m, columns = k; rows of B = k,
 *   columns = n): transposed views, the head-interleaved (B, L, 3, H, d) qkv layout and broadcast operands (batch
 *   stride 0 on A or B) need no copies.  C must not alias itself (no zero stride on an extent > 1).  nb0 * nb1 <= 65535. */
int cream_bmm_f32(float* c, const float* a, const float* b, int M, int N, int K, const int64_t* a_strides,
                  const int64_t* b_strides, const int64_t* c_strides, int nb0, int nb1, void* stream);
int cream_ln_f32_fwd(float* y, float* mean, float* rstd, const float* x, const float* gamma, const float* beta,
                     int M, int E, float eps, void* stream);
int cream_ln_f32_bwd(float* dx, float* partial, const float* dy, const float* x, const float* mean, const float* rstd,
                     const float* gamma, int M, int E, void* stream);

/* ---- active-slice gradient messages (data-parallel exchange) ------------------------------------
 * DistributedDataParallel (AutoFormer/supernet_train.py:286-289) all-reduces the FULL gradient of every
 * super weight; a sampled sub-network only writes W.grad[:rows, :cols] (Linear_super.py:71-81,
 * qkv_super.py:72-83) and every rank samples the same one (supernet_engine.py:36).  cream_slices_copy
 * gathers the active slices of one bucket into a contiguous fp32 message (to_packed != 0) or scatters
 * the reduced message back (to_packed == 0): slice i = full[r * ld + c], r < rows, c < cols, stored
 * row-major at packed + packed_off.  The job table lives in DEVICE memory (built once per bucket and
 * configuration); max_rows = the largest `rows` of the table (sizes the grid). */
typedef struct cream_slice_job {
    float* full;
    int64_t ld;
    int64_t packed_off;
    int32_t rows, cols;
} cream_slice_job;
int cream_slices_copy(const cream_slice_job* jobs_dev, int njobs, float* packed, int max_rows, int to_packed, void* stream);

/* ---- one transformer block, sequenced natively ---------------------------------------------
 * TransformerEncoderLayer.forward (AutoFormer/model/supernet_transformer.py:251-287) and its
 * autograd backward as ONE call per direction: the kernels are the ones declared above, enqueued
 * on `stream` (and, in backward, the weight-gradient GEMMs + the gradient finalisation on
 * `side_stream` behind events).  bf16 throughput mode: fp32 residual stream, bf16 GEMM operands.
 * The caller owns all memory: one flat workspace per call (sizes/offsets from *_workspace). */
typedef struct cream_block_desc {
    int32_t B, N, E, H, F;        /* batch, tokens, embed dim, heads (head dim 64), mlp hidden     */
    int32_t gh, gw, mr;           /* token grid (N = gh*gw + 1) and max_relative_position          */
    int32_t F_valid, inference;     /* inference != 0: a forward without a backward (supernet_engine.py:114-160 evaluate, the
                                       evolution search): tensors that only the backward reads (gelu'(h)) are not written.
                                       F_valid > 0: F is the sampled hidden width rounded UP to a multiple of 8 and only the
                                       first F_valid hidden units exist (the fc1 epilogue writes zeros for the rest, which
                                       makes every product over the padded columns vanish); 0: F itself is exact */
    float eps1, eps2, attn_scale;
    float reserved_f;             /* MUST be 0: every field of this struct is meaningful or reserved-as-zero — zero-initialise the
                                     struct (memset / `= {0}`) before filling it; `inference` above was a reserved field until r3 */
    /* bf16 operand copies of the SUPER weights (written by cream_adamw_step), read in place:
     * w* = (out x in) row stride ld_*, w*_t = transposed (in x out) row stride ld_*_t;
     * qkv: three de-interleaved parts [q | k | v], seg_qkv / seg_qkv_t elements apart */
    const void *wqkv, *wqkv_t, *bqkv;
    const void *wproj, *wproj_t, *bproj;
    const void *w1, *w1_t, *b1;
    const void *w2, *w2_t, *b2;
    int64_t ld_qkv, ld_qkv_t, seg_qkv, seg_qkv_t, ld_proj, ld_proj_t, ld_w1, ld_w1_t, ld_w2, ld_w2_t;
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;     /* attn_layer_norm / ffn_layer_norm (fp32)     */
    const float *tkv, *tkh, *tvv, *tvh;             /* rel_pos_embed_{k,v}.embeddings_table_{v,h}  */
    int64_t ldt;
    const void* timg;             /* bf16 operand images of the four tables (cream_attn_rpe2d_table_images layout, kept current
                                     by cream_adamw_step) or NULL: with them the forward runs the ping-pong kernel and the
                                     backward saves its image launch (round 6; NULL = the behaviour before) */
} cream_block_desc;

/* fp32 gradients of the block's parameters (super shapes; accumulated into, never overwritten) */
typedef struct cream_block_grads {
    float *wqkv, *bqkv, *wproj, *bproj, *w1, *b1, *w2, *b2;
    float *ln1_g, *ln1_b, *ln2_g, *ln2_b, *tkv, *tkh, *tvv, *tvh;
    int64_t ld_qkv, ld_proj, ld_w1, ld_w2, ldt;
} cream_block_grads;

/* Bytes of the forward workspace (kept by the caller for the backward); *off_x = block input after
 * a pending residual add (valid only if pend_f was given), *off_x1 / *off_f = the two tensors whose
 * sum x1 + s2*f is the block output — left PENDING for the next consumer (the next block's first
 * LayerNorm pass, or cream_residual_add). */
int64_t cream_block_fwd_workspace(const cream_block_desc* d, int64_t* off_x, int64_t* off_x1, int64_t* off_f);
/* x_in (M x E) fp32; pend_f (bf16, M x E) / pend_scale (B, may be NULL): pending branch of the
 * previous block, added on the fly (NULL: none); dp1: per-sample drop-path scale of the attention
 * branch (B) or NULL. */
int cream_block_fwd(const cream_block_desc* d, void* ws, const float* x_in, const void* pend_f,
                    const float* pend_scale, const float* dp1, void* stream);

/* Backward.  fws: the forward workspace; x: the block input (x_in, or fws + off_x if the forward
 * had a pending branch); dx2 (fp32) gradient of the block output; df (bf16) = s2 * dx2 = gradient
 * of the fc2 output and pb2 its column-sum partials (pb2_parts parts, pb2_pstride floats apart) —
 * both produced by whoever consumed the block's output.  Outputs in ws: dx (fp32, *off_dx) and,
 * if want_prev, df_prev = bf16(prev_scale * dx) (*off_df_prev) with its column sums as plane 2 of
 * the (cream_ln_partials() x 3 x E) partials at *off_pl1 — i.e. (df, pb2) of the previous block.
 * Parameter gradients are complete when `side_stream` has drained.
 * Ordering contract of df: when a call returns df_prev (want_prev) and the NEXT cream_block_bwd call on the same thread and
 * the same two streams is handed exactly that buffer as df, the library does not order the side stream behind it again (it
 * already is: one marker packet less per block).  The caller must therefore pass that df_prev on UNTOUCHED — a caller that
 * rewrites it on `stream` between the two calls, or produces another df at the same address, sets CREAM_REUSE_ORDER=0 in
 * the environment (always order).  The record is consumed by the next call on the thread whatever it is given. */
int64_t cream_block_bwd_workspace(const cream_block_desc* d, int64_t* off_dx, int64_t* off_df_prev, int64_t* off_pl1);
int cream_block_bwd(const cream_block_desc* d, const cream_block_grads* g, const void* fws, const float* x,
                    void* ws, const float* dx2, const void* df, const float* pb2, int pb2_parts,
                    int64_t pb2_pstride, const float* dp1, const float* prev_scale, int want_prev,
                    void* stream, void* side_stream);


/* cream_block_bwd writes the split-K partial tiles of the four weight gradients as bf16 (1) or fp32 (0); returns the
 * previous setting; on < 0 only queries.  Initial value: CREAM_WGRAD_BF16 in the environment, else 1. */
int cream_block_wgrad_bf16(int on);

/* Workspace-layout rule.  The byte size and the internal offsets of the backward workspace depend on the split counts of the
 * four weight gradients (cream_linear_wgrad_splits_bf16), i.e. on cream_gemm_tn8() and on the device's CU count: these must NOT
 * change between cream_block_bwd_workspace and the cream_block_bwd call that uses a workspace of that size (cream_block_bwd
 * recomputes the layout; a workspace sized under another mode is overrun).  cream_block_layout_epoch() returns a counter that
 * moves whenever such a switch changes value: callers that cache workspace sizes key the cache on it (cream_amd/autoformer/
 * block.py:_ws_layout does). */
int cream_block_layout_epoch(void);

/* CU budget of the persistent kernels.  Every hot kernel of the library launches one or two persistent workgroups per compute
 * unit and takes most of its LDS, so a collective kernel launched beside them (RCCL's per-step gradient all-reduce,
 * AutoFormer/supernet_train.py:286-289) only runs once a grid drains.  cream_cu_reserve(R) makes every grid of the library size
 * itself for (CUs - R) rounded down to a multiple of 8 (one share per XCD); the caller tells RCCL to use at most R channels
 * (cream_amd/comm.py: init_distributed exports NCCL_MAX_NCHANNELS / NCCL_MIN_NCHANNELS before the process group is created).
 * R < 0 queries; returns the previous reserve; moves cream_block_layout_epoch (the weight-gradient token slices follow the count).
 * cream_cu_count(): what the grids are sized for now. */
int cream_cu_reserve(int reserve);
int cream_cu_count(void);

/* Optional in-step kernel timing of the two calls above (measurement aid; no reference counterpart — the
 * reference's step is timed by `MetricLogger`, AutoFormer/lib/utils.py:58-170, at step granularity).
 * While enabled, every launch of cream_block_fwd / cream_block_bwd is bracketed by a pair of HIP events
 * recorded on the stream it is launched on (main or side), so durations are those of the real two-stream
 * step.  cream_block_prof_collect waits for the recorded events and returns, per kernel family
 * (cream_block_prof_kinds() of them, names from cream_block_prof_name), the summed duration in ms, the
 * launch count and the summed ALGORITHMIC flops / bytes; it empties the record list. */
int cream_block_prof_enable(int on);
int cream_block_prof_kinds(void);
const char* cream_block_prof_name(int kind);
int cream_block_prof_collect(double* total_ms, int64_t* launches, double* flops, double* bytes);

/* ---- RandAugment of the training recipe on the device (csrc/image_augment.hip) -----------------
 * `--aa rand-m9-mstd0.5-inc1` (AutoFormer/supernet_train.py:111; timm 0.3.2's RandAugment inside create_transform, between the
 * flip and ToTensor: lib/datasets.py:189-202).  The host draws the ops of every image (cream_amd/autoformer/data.py:
 * rand_augment_params); each op is one descriptor, Pillow's operation on the uint8 RGB image restated integer for integer (the
 * affine op in doubles, in libImaging's order of IEEE operations):
 *   NONE          identity (an op skipped by its gate)
 *   AUTOCONTRAST  ImageOps.autocontrast(cutoff 0)          EQUALIZE   ImageOps.equalize       INVERT  255 - x
 *   POSTERIZE     x & ~(2^(8 - arg) - 1), arg = bits 0..8  SOLARIZE   x < arg ? x : 255 - x, arg = threshold 0..256
 *   SOLARIZE_ADD  x < 128 ? min(255, x + arg) : x, arg 0..255
 *   COLOR / CONTRAST / BRIGHTNESS / SHARPNESS   ImageEnhance: Image.blend(degenerate, image, factor) in float32; degenerate = grey
 *                 level (19595 R + 38470 G + 7471 B + 0x8000) >> 16 / its mean over the image / 0 / ImageFilter.SMOOTH
 *   AFFINE        Image.transform(size, AFFINE, m, BICUBIC, fillcolor): output pixel (x, y) samples the input at
 *                 (m0 (x + .5) + m1 (y + .5) + m2, m3 (x + .5) + m4 (y + .5) + m5); outside the image: `fill` (R | G << 8 | B << 16).
 *                 Rotate / ShearX / ShearY / TranslateXRel / TranslateYRel are this op (Image.rotate's own matrix, from the host).
 * Per image ops_per_image descriptors, applied in order: ops[b * ops_per_image + k].  Every entry point validates the host copy
 * (unknown kind, arg out of range, non-finite factor or matrix: CREAM_ERR_BAD_ARG) before anything is enqueued; the kernels read
 * the device copy (ops_dev), which must hold the same bytes. */
#define CREAM_AUG_NONE          0
#define CREAM_AUG_AUTOCONTRAST  1
#define CREAM_AUG_EQUALIZE      2
#define CREAM_AUG_INVERT        3
#define CREAM_AUG_POSTERIZE     4
#define CREAM_AUG_SOLARIZE      5
#define CREAM_AUG_SOLARIZE_ADD  6
#define CREAM_AUG_COLOR         7
#define CREAM_AUG_CONTRAST      8
#define CREAM_AUG_BRIGHTNESS    9
#define CREAM_AUG_SHARPNESS    10
#define CREAM_AUG_AFFINE       11
#define CREAM_AUG_MAX_OPS      16  /* ops_per_image */
typedef struct cream_aug_op {
    int32_t kind;                                   /* CREAM_AUG_* */
    int32_t arg;                                    /* posterize bits / solarize threshold / solarize-add addend */
    float factor;                                   /* blend factor of the four enhance ops */
    uint32_t fill;                                  /* affine: R | G << 8 | B << 16 */
    double m[6];                                    /* affine matrix */
} cream_aug_op;
#ifdef __cplusplus
static_assert(sizeof(cream_aug_op) == 64, "cream_aug_op is 64 bytes");
#else
_Static_assert(sizeof(cream_aug_op) == 64, "cream_aug_op is 64 bytes");
#endif
/* B HWC uint8 RGB images of one size H x W (1 <= W <= 1024) -> the augmented images, dst and src packed (B, H, W, 3), not
 * overlapping; one launch per op layer.  workspace: cream_image_augment_workspace(B, H, W, ops_per_image) bytes, 16-byte aligned
 * (NULL when that is 0).  ops_per_image 0 copies nothing and returns CREAM_OK. */
int64_t cream_image_augment_workspace(int B, int H, int W, int ops_per_image);
int cream_image_augment_u8(uint8_t* dst, const uint8_t* src, int B, int H, int W, const cream_aug_op* ops, const cream_aug_op* ops_dev,
                           int ops_per_image, void* workspace, int64_t workspace_bytes, void* stream);
/* The training transform with RandAugment: crop -> bicubic resize -> mirror (the uint8 image Pillow holds there: the coefficient
 * and horizontal-pass kernels of cream_image_batch_transform, then its vertical pass writing uint8) -> the op layers -> ToTensor ->
 * Normalize -> RandomErasing (the float tail of cream_image_batch_transform, fused into the last layer).  Same conventions as
 * cream_image_batch_plan / cream_image_batch_transform; _plan_aug also validates the ops and returns a workspace size >= the plain
 * plan's.  ops_per_image == 0 is cream_image_batch_transform. */
int64_t cream_image_batch_plan_aug(cream_image_desc* descs, int B, int out_h, int out_w, const cream_aug_op* ops, int ops_per_image);
int cream_image_batch_transform_aug(float* out, const uint8_t* pixels, int64_t pixels_bytes, const cream_image_desc* descs,
                                    const cream_image_desc* descs_dev, int B, int out_h, int out_w, const float* mean,
                                    const float* stdev, const cream_aug_op* ops, const cream_aug_op* ops_dev, int ops_per_image,
                                    void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}  /* extern "C" */
#endif
#endif  /* CREAM_AMD_H_ */

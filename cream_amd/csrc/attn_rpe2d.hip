// attn_rpe2d.hip — fused multi-head attention with AutoFormer's 2-D relative position bias
// on keys and values, forward and backward, for gfx950 (MI355X).
//
// Reference semantics (AutoFormer/model/module/multihead_super.py:135-154),
// per (batch b, head h), head_dim 64, N tokens (token 0 = class token, then a gh x gw grid):
//     Lv = q Tkv^T ; Lh = q Tkh^T                                  (N x nb bucket lookups)
//     A[i,j] = scale * ( q_i.k_j + Lv[i, iv[i,j]] + Lh[i, ih[i,j]] )
//     P = softmax_j(A)
//     Sv[i,u] = sum_{j: iv[i,j]=u} P[i,j] ; Sh likewise
//     O_i = sum_j P[i,j] v_j + Sv[i,:] Tvv + Sh[i,:] Tvh
// Nothing of size N^2 touches HBM.  One workgroup = one (b,h); wave w owns the 32-query
// tile w and keeps the whole row block of scores in registers (N <= 256), so the softmax is
// exact (no online rescaling).  The bias gather / slot sums ride on the MFMAs through the
// one-hot extension described in attn_common.hpp.  Operands shared by the waves of a
// workgroup (K, V, Q, dO, side buffers) are streamed through LDS tile by tile (full lines,
// fetched once per workgroup, two 4-wave staging groups); transposed tiles for the products
// that contract over tokens (V^T, K^T, Q^T, dO^T) are produced by the staging stores.  LDS also
// holds the bucket tables as bf16 operands, the one-hot key operands of the fast geometry and
// the per-wave scratch of the slot <-> bucket shifts.  The AutoFormer geometry (14 x 14 grid,
// max_relative_position 14, bf16) has its own kernels and instantiation (FAST): the kernels were
// VALU-issue-bound on index arithmetic, see attn_common.hpp and DESIGN.md 4.2.
//
// dtype = bf16 (throughput mode: bf16 operands, fp32 accumulation/softmax) or fp32 (parity
// mode: v_mfma_f32_32x32x2_f32, exact fp32 products) — one code path, Tr<T> traits.
//
// This file: the launchers, the switches and the C ABI.  The kernels, one header each:
//   attn_rpe2d_tile.hpp     argument structs, phase stamps, the pieces the tile-streamed kernels share
//   attn_rpe2d_fwd.hpp      tile-streamed forward           attn_rpe2d_bwd.hpp   two-launch backward (dQ, then dK / dV)
//   attn_rpe2d_fwd14.hpp    14 x 14 forward, K and V whole in LDS (registers-staged)
//   attn_rpe2d_whole14.hpp  what the whole-matrix kernels of the 14 x 14 geometry share (LDS layout, table images, DMA)
//   attn_rpe2d_fwd2.hpp     ping-pong forward (default)     attn_rpe2d_bwd1.hpp / _bwd2.hpp   one-pass backward (bwd2: default)
#include <hip/hip_runtime.h>
#include <hip/hip_bfloat16.h>
#include <stdint.h>
#include <stdlib.h>

#include "attn_rpe2d_tile.hpp"
#include "attn_rpe2d_fwd.hpp"
#include "attn_rpe2d_fwd14.hpp"
#include "attn_rpe2d_bwd.hpp"
#include "attn_rpe2d_whole14.hpp"
#include "attn_rpe2d_fwd2.hpp"
#include "attn_rpe2d_bwd1.hpp"
#include "attn_rpe2d_bwd2.hpp"
#include "cream_amd.h"
#include "launch_ev.hpp"
#include "cu_budget.hpp"
#include "env_switch.hpp"

namespace {
using namespace cream;

// one persistent workgroup per CU (the kernels' LDS footprints allow exactly one), forward and backward
int persistent_grid() { return cream::cu_count(); }

// launch a persistent kernel over the B * H items of `a` (FwdArgs / BwdArgs): min(items, CUs) workgroups walk them
template <typename K, typename Args, typename... Extra>
int launch_items(K kern, int threads, size_t lds, hipStream_t st, const Args& a, int B, Extra... extra) {
    if (!cream::raise_dynamic_lds(kern, 160 * 1024)) return CREAM_ERR_LAUNCH;
    Args aa = a;
    aa.nitems = B * a.H;
    const int grid = aa.nitems < persistent_grid() ? aa.nitems : persistent_grid();
    CREAM_LAUNCH(kern, dim3(grid), dim3(threads), lds, st, aa, extra...);
    return hipGetLastError() == hipSuccess ? CREAM_OK : CREAM_ERR_LAUNCH;
}

bool fast_geometry(const RelGeom& G) { return G.n == 197 && G.gh == G14 && G.gw == G14 && G.mr == G14; }

template <typename T, int NT, bool DROP = false>
int launch_fwd_nt(const FwdArgs& a, int B, hipStream_t st) {
    const int waves = a.NP / 32 < 4 ? 4 : a.NP / 32;
    return launch_items(attn_rpe2d_fwd_kernel<T, NT, DROP>, waves * 64, fwd_lds_bytes<T>(a.NP, waves), st, a, B);
}

// 1: the ping-pong online-softmax forward (attn_rpe2d_fwd2.hpp) whenever the caller hands over the table images
// (AutoFormer geometry, bf16); 0: attn_rpe2d_fwd14.  CREAM_ATTN_FWD2 in the environment sets the initial value.
EnvSwitch g_fwd2{"CREAM_ATTN_FWD2", 1, norm_bool};

int launch_fwd2(const FwdArgs& a, int B, hipStream_t st) {
    return launch_items(fwd2::attn_rpe2d_fwd2_kernel, fwd2::F2_THREADS, fwd2::F2_LDS_B, st, a, B, reinterpret_cast<const short*>(a.timg));
}

int launch_fwd14(const FwdArgs& a, int B, hipStream_t st) {
    return launch_items(attn_rpe2d_fwd14_kernel, W14_THREADS, fwd14_lds_bytes(), st, a, B);
}

template <typename T>
int launch_fwd(const FwdArgs& a, int B, hipStream_t st) {
    const int nt = a.NP / 32;
    if (a.drop_thr) {        // attention dropout: the tile-streamed kernel for every geometry (the score row block is in registers when the mask applies)
        if (nt <= 2) return launch_fwd_nt<T, 2, true>(a, B, st);
        if (nt <= 4) return launch_fwd_nt<T, 4, true>(a, B, st);
        if (nt <= 7) return launch_fwd_nt<T, 7, true>(a, B, st);
        return launch_fwd_nt<T, 8, true>(a, B, st);
    }
    if (nt <= 2) return launch_fwd_nt<T, 2>(a, B, st);
    if (nt <= 4) return launch_fwd_nt<T, 4>(a, B, st);
    if constexpr (sizeof(typename Tr<T>::elem) == 2) {
        // (measured and dropped: an instantiation of the tile-streamed kernel for this geometry with compile-time shapes and
        //  one-hot operands in LDS: 46.5 us against 40.6 us at B = 128, H = 6; 10.56 vs 10.48 ms per step in a same-box A/B x3)
        if (fast_geometry(a.G)) return a.timg && g_fwd2.get() ? launch_fwd2(a, B, st) : launch_fwd14(a, B, st);
    }
    if (nt <= 7) return launch_fwd_nt<T, 7>(a, B, st);
    return launch_fwd_nt<T, 8>(a, B, st);
}

template <typename T, bool FAST, bool DROP = false>
int launch_bwd_impl(const BwdArgs& a, int B, hipStream_t st) {
    auto kq = attn_rpe2d_bwd_q_kernel<T, FAST, DROP>;
    auto kkv = attn_rpe2d_bwd_kv_kernel<T, DROP>;
    if (!cream::raise_dynamic_lds(kq, 160 * 1024)) return CREAM_ERR_LAUNCH;
    BwdArgs aa = a;
    aa.nitems = B * a.H;
    const int pgrid = aa.nitems < persistent_grid() ? aa.nitems : persistent_grid();
    // a plain launch: the completion event armed by block_seq.cpp rides on the LAST kernel of the operator
    hipLaunchKernelGGL(kq, dim3(pgrid), dim3(512), bwd_q_lds_bytes<T>(a.NP, a.NP / 32, FAST), st, aa);
    if (hipGetLastError() != hipSuccess) return CREAM_ERR_LAUNCH;
#ifdef PROBE_SKIP_KV                     // tools/probes/attn_probe.hip: keep the dQ kernel's phase stamps
    (void)kkv;
    return CREAM_OK;
#endif
    return launch_items(kkv, 512, bwd_kv_lds_bytes<T>(a.NP), st, a, B);
}

// The backward of the AutoFormer geometry in bf16: 0 = the two-launch backward (what every other geometry and fp32 run);
// 1 = the one-pass kernel with both roles on every wave (attn_rpe2d_bwd1.hpp, 7 waves); 2 = the one-pass kernel with the roles
// on separate waves and the table gradients in registers (attn_rpe2d_bwd2.hpp, 12 waves) — the DEFAULT: 91.6 against 102.6 us
// alone at B = 128, H = 6, same-call step A/B x3 8.475 -> 8.321 ms (profiles/r06_attn_bwd2.md).
// CREAM_ATTN_BWD1 in the environment sets the initial value; cream_attn_rpe2d_bwd_mode() switches it (A/B runs).
EnvSwitch g_bwd_onepass{"CREAM_ATTN_BWD1", 2, [](int m) { return m > 2 ? 1 : m; }};

// the side buffer `dlt` of the two-launch path (B*H*64*NP elements, far more than the 32 KB needed) carries the bf16
// operand images of the four tables
int launch_bwd1(const BwdArgs& a, int B, hipStream_t st) {
    const bool roles_apart = g_bwd_onepass.get() == 2;
    BwdArgs aa = a;
    aa.stagger = 0;                                  // (de-phasing the workgroups' first items was measured: no gain, profiles/r04_attn_bwd1.md)
    if (roles_apart) { static const int stg = getenv("CREAM_ATTN_BWD_STAGGER") ? atoi(getenv("CREAM_ATTN_BWD_STAGGER")) : 0; aa.stagger = stg; }   // (< 0: items in (b, h) order)
    const short* img = reinterpret_cast<const short*>(a.timg);
    if (!img) {                                      // no images from the caller: built into the side buffer, one more launch
        short* own = reinterpret_cast<short*>(a.dlt);
        hipLaunchKernelGGL(whole14::table_images_kernel, dim3(8), dim3(256), 0, st, own, a.tkv, a.tkh, a.tvv, a.tvh, a.ldt, a.nb);
        if (hipGetLastError() != hipSuccess) return CREAM_ERR_LAUNCH;
        img = own;
    }
    if (roles_apart) return launch_items(bwd2::attn_rpe2d_bwd2_kernel, bwd2::THREADS, bwd2::LDS_B, st, aa, B, img);
    return launch_items(bwd1::attn_rpe2d_bwd1_kernel, whole14::THREADS, whole14::LDS_B, st, aa, B, img);
}

template <typename T>
int launch_bwd(const BwdArgs& a, int B, hipStream_t st) {
    if (a.drop_thr) return launch_bwd_impl<T, false, true>(a, B, st);       // attention dropout: the two-launch backward regenerates the mask
    if constexpr (sizeof(typename Tr<T>::elem) == 2) {
        if (fast_geometry(a.G)) {
            if (g_bwd_onepass.get() && (size_t)B * a.H * 64 * a.NP >= (size_t)whole14::IMG_ELEMS) return launch_bwd1(a, B, st);
            return launch_bwd_impl<T, true>(a, B, st);
        }
    }
    return launch_bwd_impl<T, false>(a, B, st);
}

bool geom_ok(int N, int gh, int gw, int mr, int nb) {
    return N >= 1 && N <= 256 && gh >= 0 && gw >= 1 && gh * gw + 1 == N && gh < CB && gw <= 32 - CB && mr >= 0 &&
           nb == 2 * mr + 2 && nb <= 32;
}

}  // namespace

extern "C" {

int cream_attn_rpe2d_padded_len(int N) { return N <= 0 ? 0 : ((N + 31) / 32) * 32; }

int cream_attn_rpe2d_bwd_mode(int onepass) { return g_bwd_onepass.set(onepass); }

int cream_attn_rpe2d_dtab_parts(int B, int H)
{
    if (B <= 0 || H <= 0) return 0;
    const int64_t items = (int64_t)B * H;
    return (int)(items < persistent_grid() ? items : persistent_grid());
}

int cream_attn_rpe2d_fwd_mode(int on) { return g_fwd2.set(on); }

int64_t cream_attn_rpe2d_table_image_bytes(void) { return (int64_t)whole14::IMG_ELEMS * 2; }

int cream_attn_rpe2d_table_images(void* img, const float* tkv, const float* tkh, const float* tvv, const float* tvh, int ldt,
                                  int mr, void* stream)
{
    if (!img || !tkv || !tkh || !tvv || !tvh || ldt < 64 || mr < 0 || 2 * mr + 2 > 32 || ((uintptr_t)img) % 16) return CREAM_ERR_BAD_ARG;
    hipLaunchKernelGGL(whole14::table_images_kernel, dim3(8), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<short*>(img), tkv, tkh,
                       tvv, tvh, ldt, 2 * mr + 2);
    return hipGetLastError() == hipSuccess ? CREAM_OK : CREAM_ERR_LAUNCH;
}

int cream_attn_rpe2d_fwd(void* out, float* lse, void* sp, const void* q, const void* k, const void* v,
                         int64_t sb, int64_t sn, int64_t sh, const float* tkv, const float* tkh,
                         const float* tvv, const float* tvh, int ldt, int B, int H, int N, int gh, int gw,
                         int mr, float scale, int dtype, void* stream)
{
    return cream_attn_rpe2d_fwd_img(out, lse, sp, q, k, v, sb, sn, sh, tkv, tkh, tvv, tvh, ldt, nullptr, B, H, N, gh, gw, mr, scale,
                                    dtype, stream);
}

int cream_attn_rpe2d_fwd_img(void* out, float* lse, void* sp, const void* q, const void* k, const void* v,
                             int64_t sb, int64_t sn, int64_t sh, const float* tkv, const float* tkh,
                             const float* tvv, const float* tvh, int ldt, const void* timg, int B, int H, int N, int gh, int gw,
                             int mr, float scale, int dtype, void* stream)
{
    return cream_attn_rpe2d_fwd_drop(out, lse, sp, q, k, v, sb, sn, sh, tkv, tkh, tvv, tvh, ldt, timg, B, H, N, gh, gw, mr, scale,
                                     0.f, 0u, dtype, stream);
}

int cream_attn_rpe2d_fwd_drop(void* out, float* lse, void* sp, const void* q, const void* k, const void* v,
                              int64_t sb, int64_t sn, int64_t sh, const float* tkv, const float* tkh,
                              const float* tvv, const float* tvh, int ldt, const void* timg, int B, int H, int N, int gh, int gw,
                              int mr, float scale, float dropout_p, uint32_t dropout_seed, int dtype, void* stream)
{
    if (B < 0 || H < 0) return CREAM_ERR_BAD_ARG;
    if (!(dropout_p >= 0.f) || dropout_p >= 1.f) return CREAM_ERR_BAD_ARG;
    if (B == 0 || H == 0) return CREAM_OK;
    if (!out || !lse || !q || !k || !v || !tkv || !tkh || !tvv || !tvh) return CREAM_ERR_BAD_ARG;     // (sp == NULL: forward only)
    if (!geom_ok(N, gh, gw, mr, 2 * mr + 2)) return CREAM_ERR_TOO_LARGE;
    if (ldt < 64) return CREAM_ERR_BAD_ARG;
    const int esz = dtype == CREAM_F32 ? 4 : 2;
    // 16-byte vector loads of operand rows
    if ((sb * esz) % 16 || (sn * esz) % 16 || (sh * esz) % 16) return CREAM_ERR_BAD_ARG;
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) % 16) return CREAM_ERR_BAD_ARG;
    if (ldt % 4 || ((uintptr_t)tkv | (uintptr_t)tkh) % 16 || ((uintptr_t)timg) % 16) return CREAM_ERR_BAD_ARG;
    FwdArgs a;
    a.timg = timg;
    a.q = q; a.k = k; a.v = v; a.sb = sb; a.sn = sn; a.sh = sh;
    a.out = out; a.lse = lse; a.sp = sp;
    a.tkv = tkv; a.tkh = tkh; a.tvv = tvv; a.tvh = tvh; a.ldt = ldt; a.nb = 2 * mr + 2;
    a.H = H; a.NP = cream_attn_rpe2d_padded_len(N);
    a.G = RelGeom{N, gh, gw, mr};
    a.scale = scale;
    a.drop_thr = drop_threshold(dropout_p);
    a.drop_seed = dropout_seed;
    a.drop_scale = 1.f / (1.f - dropout_p);
    hipStream_t st = (hipStream_t)stream;
    switch (dtype) {
        case CREAM_BF16: return launch_fwd<hip_bfloat16>(a, B, st);
        case CREAM_F32: return launch_fwd<float>(a, B, st);
        default: return CREAM_ERR_BAD_DTYPE;
    }
}

int cream_attn_rpe2d_bwd(void* dq, void* dk, void* dv, int64_t dsb, int64_t dsn, int64_t dsh, float* dtab,
                         void* dlt, void* qe, void* de, float* delta,
                         const void* dout, const void* out, const float* lse, const void* sp,
                         const void* q, const void* k, const void* v, int64_t sb, int64_t sn, int64_t sh,
                         const float* tkv, const float* tkh, const float* tvv, const float* tvh, int ldt,
                         int B, int H, int N, int gh, int gw, int mr, float scale, int dtype, void* stream)
{
    return cream_attn_rpe2d_bwd_img(dq, dk, dv, dsb, dsn, dsh, dtab, dlt, qe, de, delta, dout, out, lse, sp, q, k, v, sb, sn, sh, tkv, tkh,
                                    tvv, tvh, ldt, nullptr, B, H, N, gh, gw, mr, scale, dtype, stream);
}

int cream_attn_rpe2d_bwd_img(void* dq, void* dk, void* dv, int64_t dsb, int64_t dsn, int64_t dsh, float* dtab,
                             void* dlt, void* qe, void* de, float* delta,
                             const void* dout, const void* out, const float* lse, const void* sp,
                             const void* q, const void* k, const void* v, int64_t sb, int64_t sn, int64_t sh,
                             const float* tkv, const float* tkh, const float* tvv, const float* tvh, int ldt, const void* timg,
                             int B, int H, int N, int gh, int gw, int mr, float scale, int dtype, void* stream)
{
    return cream_attn_rpe2d_bwd_drop(dq, dk, dv, dsb, dsn, dsh, dtab, dlt, qe, de, delta, dout, out, lse, sp, q, k, v, sb, sn, sh, tkv,
                                     tkh, tvv, tvh, ldt, timg, B, H, N, gh, gw, mr, scale, 0.f, 0u, dtype, stream);
}

int cream_attn_rpe2d_bwd_drop(void* dq, void* dk, void* dv, int64_t dsb, int64_t dsn, int64_t dsh, float* dtab,
                              void* dlt, void* qe, void* de, float* delta,
                              const void* dout, const void* out, const float* lse, const void* sp,
                              const void* q, const void* k, const void* v, int64_t sb, int64_t sn, int64_t sh,
                              const float* tkv, const float* tkh, const float* tvv, const float* tvh, int ldt, const void* timg,
                              int B, int H, int N, int gh, int gw, int mr, float scale, float dropout_p, uint32_t dropout_seed,
                              int dtype, void* stream)
{
    if (B < 0 || H < 0) return CREAM_ERR_BAD_ARG;
    if (!(dropout_p >= 0.f) || dropout_p >= 1.f) return CREAM_ERR_BAD_ARG;
    if (B == 0 || H == 0) return CREAM_OK;
    if (!dq || !dk || !dv || !dtab || !dlt || !qe || !de || !delta || !dout || !out || !lse || !sp || !q || !k ||
        !v || !tkv || !tkh || !tvv || !tvh)
        return CREAM_ERR_BAD_ARG;
    if (!geom_ok(N, gh, gw, mr, 2 * mr + 2)) return CREAM_ERR_TOO_LARGE;
    if (ldt < 64 || ldt % 4) return CREAM_ERR_BAD_ARG;
    const int esz = dtype == CREAM_F32 ? 4 : 2;
    if ((sb * esz) % 16 || (sn * esz) % 16 || (sh * esz) % 16 || (dsb * esz) % 16 || (dsn * esz) % 16 ||
        (dsh * esz) % 16)
        return CREAM_ERR_BAD_ARG;
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv |
         (uintptr_t)dout | (uintptr_t)out | (uintptr_t)sp | (uintptr_t)dlt | (uintptr_t)qe | (uintptr_t)de |
         (uintptr_t)dtab | (uintptr_t)tkv | (uintptr_t)tkh | (uintptr_t)tvv | (uintptr_t)tvh | (uintptr_t)timg) % 16)
        return CREAM_ERR_BAD_ARG;
    BwdArgs a{};
    a.timg = timg;
    a.q = q; a.k = k; a.v = v; a.sb = sb; a.sn = sn; a.sh = sh;
    a.dq = dq; a.dk = dk; a.dv = dv; a.dsb = dsb; a.dsn = dsn; a.dsh = dsh;
    a.dout = dout; a.out = out; a.lse = lse; a.sp = sp;
    a.dlt = dlt; a.qe = qe; a.de = de; a.delta = delta; a.dtab = dtab;
    a.tkv = tkv; a.tkh = tkh; a.tvv = tvv; a.tvh = tvh; a.ldt = ldt; a.nb = 2 * mr + 2;
    a.H = H; a.NP = cream_attn_rpe2d_padded_len(N);
    a.G = RelGeom{N, gh, gw, mr};
    a.scale = scale;
    a.drop_thr = drop_threshold(dropout_p);
    a.drop_seed = dropout_seed;
    a.drop_scale = 1.f / (1.f - dropout_p);
    hipStream_t st = (hipStream_t)stream;
    switch (dtype) {
        case CREAM_BF16: return launch_bwd<hip_bfloat16>(a, B, st);
        case CREAM_F32: return launch_bwd<float>(a, B, st);
        default: return CREAM_ERR_BAD_DTYPE;
    }
}

}  // extern "C"

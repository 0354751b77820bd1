// attn_rpe2d_fwd.hpp — the tile-streamed forward of attn_rpe2d.hip: every geometry and dtype, K and V streamed through
// LDS one 32-token tile at a time (the AutoFormer geometry in bf16 runs attn_rpe2d_fwd2.hpp or attn_rpe2d_fwd14.hpp).
#pragma once
#include "attn_rpe2d_tile.hpp"

namespace {

// LDS: [2 x max(K tile, V^T tile)] | value tables^T [64][tp] | key table rows [64][tp] (bf16) | masks [NP] | scratch
template <typename T> size_t fwd_lds_bytes(int NP, int waves) {
    using E = typename Tr<T>::elem;
    const size_t tile = rm_tile_bytes<T>(64) > t_tile_bytes<T>() ? rm_tile_bytes<T>(64) : t_tile_bytes<T>();
    return 2 * tile + (size_t)(64 + tabr_rows<T>(2)) * table_pitch<T>() * sizeof(E) + (size_t)NP * 4 +
           (size_t)waves * 32 * LP * 4;
}

template <typename T, int NT, bool DROP = false>
__global__ __launch_bounds__((NT < 4 ? 4 : NT) * 64) void attn_rpe2d_fwd_kernel(const FwdArgs a) {
    using TT = Tr<T>;
    using E = typename TT::elem;
    using F = typename TT::frag;
    constexpr int KI = TT::KI, EPL = TT::EPL, S64 = 64 / KI, S32 = 32 / KI;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const RelGeom G = a.G;
    const int N = G.n, NP = a.NP;
    const int nt = NP >> 5;
    constexpr int tp = table_pitch<T>(), kp = rm_pitch<T>(64), vp = t_pitch<T>();
    constexpr size_t tile_b = rm_tile_bytes<T>(64) > t_tile_bytes<T>() ? rm_tile_bytes<T>(64) : t_tile_bytes<T>();
    E* buf0 = reinterpret_cast<E*>(smem);
    E* buf1 = reinterpret_cast<E*>(smem + tile_b);
    E* tvt = reinterpret_cast<E*>(smem + 2 * tile_b);                     // value tables^T [64][tp]
    E* tkr = tvt + 64 * tp;                                               // key table rows [64][tp] (bf16)
    uint32_t* masks = reinterpret_cast<uint32_t*>(tkr + tabr_rows<T>(2) * tp);   // [NP]
    float* scratch = reinterpret_cast<float*>(masks + NP);                // [waves][32][LP]

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, g = lane >> 5, c32 = lane & 31;
    const bool active = wave < nt;                                        // waves beyond the query tiles only help staging
    const int qi = wave * 32 + c32;
    const bool qok = qi < N;
    const int qr = qi > 0 ? (qi - 1) / G.gw : 0, qc = qi > 0 ? (qi - 1) - qr * G.gw : 0;

    // ---- once per workgroup: tables, key slot masks (the same for every (b, h)) ------------------------------
    // The workgroup is PERSISTENT: it walks (b, h) items blockIdx.x, + gridDim.x, ... so that this setup — a
    // quarter of a one-item workgroup's time, all CUs bursting on the tables at once — is paid once per CU.
    {
        TabRegs rv, rk;
        tab_load(rv, a.tvv, a.tvh, a.ldt, a.nb);
        if constexpr (tables_in_lds<T>()) tab_load(rk, a.tkv, a.tkh, a.ldt, a.nb);
        tab_store_T<T>(rv, tvt);
        if constexpr (tables_in_lds<T>()) tab_store_R<T>(rk, tkr);
    }
    for (int j = threadIdx.x; j < NP; j += blockDim.x) masks[j] = key_mask(j, G);

    for (int item = blockIdx.x; item < a.nitems; item += gridDim.x) {
    const int b = item / a.H, h = item - b * a.H;
    const int64_t base = (int64_t)b * a.sb + (int64_t)h * a.sh;
    const E* qp = reinterpret_cast<const E*>(a.q) + base;
    const E* kpg = reinterpret_cast<const E*>(a.k) + base;
    const E* vpg = reinterpret_cast<const E*>(a.v) + base;

    PROF_DECL
    PROF_MARK();
    F qb[S64];
    load_row<T>(qb, qp + (int64_t)min(qi, N - 1) * a.sn, g);
    // K tiles 0..nt-1 and then V tiles 0..nt-1 form ONE stream of 2*nt staged tiles: tile u is
    // loaded into register set u % PF a full PF tile-iterations before it is written to LDS buffer
    // u & 1 (one iteration of ~1.3k cycles is shorter than an HBM round trip under load: with
    // a single tile in flight every iteration ended in a wait for memory)
    // ONLINE (row blocks of 5+ key tiles): the tiles alternate K_0 V_0 K_1 V_1 ... and the softmax runs online, tile by
    // tile, against a running maximum — the whole score row block (NT x 16 registers beside 48 of accumulators, the
    // operand fragments and the tiles in flight) does not fit the 256 registers of a wave at two waves per SIMD: the
    // exact-softmax form of this kernel kept 690-1050 bytes per lane in scratch at NT = 7 / 8.
    constexpr bool ONLINE = NT > 4;
    // (ONLINE: K tiles travel in ring[0], V tiles in ring[1] — static register indices under a loop that is NOT unrolled)
    constexpr int PF = ONLINE ? 2 : (sizeof(E) == 2 ? 3 : 1);      // exact form in fp32: tiles are twice the registers, one in flight
    TileRegs<T, 32, 64> ring[PF];
    auto issue = [&](int u) {
        if constexpr (ONLINE) {
            if (u < 2 * nt) {
                if (u & 1) tile_load<T, 32, 64>(ring[PF - 1], vpg, a.sn, (u >> 1) * 32, N);
                else tile_load<T, 32, 64>(ring[0], kpg, a.sn, (u >> 1) * 32, N);
            }
        } else {
        if (u < nt) tile_load<T, 32, 64>(ring[u % PF], kpg, a.sn, u * 32, N);
        else if (u < 2 * nt) tile_load<T, 32, 64>(ring[u % PF], vpg, a.sn, (u - nt) * 32, N);
        }
    };
    auto commit = [&](int u) {
        E* dst = (u & 1) ? buf1 : buf0;
        const bool is_k = ONLINE ? !(u & 1) : u < nt;
        if (u >= 2 * nt) return;
        if constexpr (ONLINE) {
            if (is_k) tile_store<T, 32, 64, true, false>(ring[0], buf0, kp, nullptr, 0);
            else if constexpr (sizeof(E) == 2) tile_store<T, 32, 64, true, false>(ring[PF - 1], buf1, kp, nullptr, 0);
            else tile_store<T, 32, 64, false, true>(ring[PF - 1], nullptr, 0, buf1, vp);
            return;
        }
        if (is_k) tile_store<T, 32, 64, true, false>(ring[u % PF], dst, kp, nullptr, 0);
        else {
            // V tiles: bf16 keeps them row-major (the P.V product reads them through ds_read_b64_tr_b16)
            if constexpr (sizeof(E) == 2) tile_store<T, 32, 64, true, false>(ring[u % PF], dst, kp, nullptr, 0);
            else tile_store<T, 32, 64, false, true>(ring[u % PF], nullptr, 0, dst, vp);
        }
    };
#pragma unroll
    for (int u = 0; u < PF; ++u) issue(u);

    // ---- item prologue: first K tile (the barrier also separates this item's staging and scratch use from the
    // previous item's last tile and epilogue, and publishes the once-per-workgroup setup) ---------------------
    __syncthreads();
    commit(0);
    issue(PF);
    __syncthreads();
    PROF_MARK();

    // ---- this wave's query tile: bucket lookups -> slot extension ---------------------------
    float* scr = scratch + wave * 32 * LP;
    if (!qok) zero_frags<T, S64>(qb);
    F qe[S32];
    if (active) {
        table_lookups<T>(scr, qb, tkr, a.tkv, a.tkh, a.ldt, a.nb, lane);
        wave_lds_fence();
        build_ext<T>(qe, scr, lane, qi, qr, qc, G);
    }
    PROF_MARK();

    f32x16 o[2] = {f32x16{}, f32x16{}};
    f32x16 ox = {};
    float inv_l;
    if constexpr (ONLINE) {
    // ---- one pass over (K_t, V_t): scores of 32 keys, online softmax, [O | slot sums]^T += [V | one-hot]^T . P^T --------
    const float sc = a.scale * LOG2E;
    float m_run = -INFINITY, l = 0.f;                  // running maximum of the raw scores / this lane's half of the running sum
#pragma unroll 1
    for (int t = 0; t < nt; ++t)
        {
            f32x16 st = {};
            if (active) {
#pragma unroll
                for (int ks = 0; ks < S64; ++ks)
                    st = TT::mma(TT::load(buf0 + c32 * kp + ks * KI + g * EPL), qb[ks], st);
                const uint32_t km = masks[t * 32 + c32];
#pragma unroll
                for (int ks = 0; ks < S32; ++ks) st = TT::mma(TT::onehot_row(km, ks, g), qe[ks], st);
            }
            commit(2 * t + 1);                         // V_t
            __syncthreads();
            issue(2 * t + 1 + PF);
#pragma unroll
            for (int r = 0; r < 16; ++r)               // keys >= N (they exist only in the last tile)
                if (t * 32 + acc_row(r, g) >= N) st[r] = -INFINITY;
            float m4[4] = {st[0], st[1], st[2], st[3]};
#pragma unroll
            for (int r = 4; r < 16; ++r) m4[r & 3] = fmaxf(m4[r & 3], st[r]);
            float mt = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
            mt = fmaxf(mt, __shfl_xor(mt, 32));
            const float m_new = fmaxf(m_run, mt);      // (every tile holds a key < N: finite from the first tile on)
            const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * sc);      // first tile: exp2(-inf) = 0 on zeros
            const float msc = m_new * sc;
            m_run = m_new;
            float l4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(st[r], sc, -msc));
                st[r] = p;
                l4[r & 3] += p;
            }
            l = __builtin_fmaf(l, alpha, (l4[0] + l4[1]) + (l4[2] + l4[3]));
#pragma unroll
            for (int r = 0; r < 16; ++r) { o[0][r] *= alpha; o[1][r] *= alpha; ox[r] *= alpha; }
            if constexpr (DROP) {                      // the normaliser is the undropped sum
                const uint32_t dkey = drop_key(a.drop_seed, item);
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    st[r] = drop_keep(dkey, qi, t * 32 + acc_row(r, g), a.drop_thr) ? st[r] * a.drop_scale : 0.f;
            }
            if (active) {
#pragma unroll
                for (int st2 = 0; st2 < S32; ++st2) {
                    const F pb = TT::from_acc(st, st2);
                    o[0] = TT::mma(perm_operand<T>(buf1, kp, buf1, vp, 0, st2, lane), pb, o[0]);
                    o[1] = TT::mma(perm_operand<T>(buf1, kp, buf1, vp, 1, st2, lane), pb, o[1]);
                    ox = TT::mma(TT::onehot_perm(masks + t * 32, st2, g, c32), pb, ox);
                }
            }
            if (t + 1 < nt) {
                commit(2 * t + 2);                     // K_{t+1}
                __syncthreads();
                issue(2 * t + 2 + PF);
            }
        }
    l += __shfl_xor(l, 32);
    inv_l = 1.f / l;
    if (active && qok && g == 0)
        a.lse[((int64_t)b * a.H + h) * N + qi] = (m_run * sc + log2f(l)) * (1.f / LOG2E);
    PROF_MARK();
    } else {
    // ---- S^T tiles: scores of all keys against this wave's 32 queries (K streamed) ------
    f32x16 s[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        s[t] = f32x16{};
        if (t < nt) {
            const E* kb = (t & 1) ? buf1 : buf0;
            if (active) {
#pragma unroll
                for (int ks = 0; ks < S64; ++ks)
                    s[t] = TT::mma(TT::load(kb + c32 * kp + ks * KI + g * EPL), qb[ks], s[t]);
                const uint32_t km = masks[t * 32 + c32];
#pragma unroll
                for (int ks = 0; ks < S32; ++ks) s[t] = TT::mma(TT::onehot_row(km, ks, g), qe[ks], s[t]);
            }
            commit(t + 1);                             // the last iteration commits V^T tile 0
            __syncthreads();
            issue(t + 1 + PF);
        }
    }
    PROF_MARK();

    // ---- softmax over keys (in-lane + one exchange with the partner lane) ---------------
    // keys >= N exist only in the last tile
#pragma unroll
    for (int t = 0; t < NT; ++t)
        if (t == nt - 1) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (t * 32 + acc_row(r, g) >= N) s[t][r] = -INFINITY;
        }
    // four independent max / sum chains (a single chain of 112 dependent ops is latency-bound)
    float m4[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int t = 0; t < NT; ++t)
        if (t < nt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) m4[r & 3] = fmaxf(m4[r & 3], s[t][r]);
        }
    float m = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
    m = fmaxf(m, __shfl_xor(m, 32));
    const float sc = a.scale * LOG2E;
    const float msc = m * sc;
    float l4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NT; ++t)
        if (t < nt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[t][r], sc, -msc));
                s[t][r] = p;
                l4[r & 3] += p;
            }
        }
    float l = (l4[0] + l4[1]) + (l4[2] + l4[3]);
    l += __shfl_xor(l, 32);
    inv_l = 1.f / l;
    if (active && qok && g == 0)
        a.lse[((int64_t)b * a.H + h) * N + qi] = (msc + log2f(l)) * (1.f / LOG2E);
    if constexpr (DROP) {                          // the normaliser above is the undropped sum; V product and slot sums take the dropped map
        const uint32_t dkey = drop_key(a.drop_seed, item);
#pragma unroll
        for (int t = 0; t < NT; ++t)
            if (t < nt) {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    s[t][r] = drop_keep(dkey, qi, t * 32 + acc_row(r, g), a.drop_thr) ? s[t][r] * a.drop_scale : 0.f;
            }
    }
    PROF_MARK();

    // ---- [O | slot sums]^T = [V | one-hot]^T . P^T   (V^T streamed) -------------------------
#pragma unroll
    for (int t = 0; t < NT; ++t)
        if (t < nt) {
            const E* vb = ((nt + t) & 1) ? buf1 : buf0;
            if (active) {
#pragma unroll
                for (int st2 = 0; st2 < S32; ++st2) {
                    const F pb = TT::from_acc(s[t], st2);
                    o[0] = TT::mma(perm_operand<T>(vb, kp, vb, vp, 0, st2, lane), pb, o[0]);
                    o[1] = TT::mma(perm_operand<T>(vb, kp, vb, vp, 1, st2, lane), pb, o[1]);
                    ox = TT::mma(TT::onehot_perm(masks + t * 32, st2, g, c32), pb, ox);
                }
            }
            if (t + 1 < nt) {
                commit(nt + t + 1);
                __syncthreads();
                issue(nt + t + 1 + PF);
            }
        }
    }   // exact softmax over the whole row block (NT <= 4)
    if (active) {
#pragma unroll
    for (int r = 0; r < 16; ++r) { o[0][r] *= inv_l; o[1][r] *= inv_l; ox[r] *= inv_l; }
    PROF_MARK();

    // ---- value-side relative position term: slot sums -> bucket sums -> . tables ---------
    float bk[32];
    slots_to_buckets(bk, scr, ox, lane, qi, qr, qc, G);
    // S'^T (64 buckets x NP queries) for backward (dTvv / dTvh)
    if (a.sp) store_buckets_T<T>(reinterpret_cast<E*>(a.sp) + ((int64_t)b * a.H + h) * 64 * NP + qi, NP, bk, g);   // (NULL: no backward will follow)
    add_bucket_product<T>(o, tvt, bk, lane);
    PROF_MARK();

    // ---- store O (b, n, h, :) ----------------------------------------------------------------
    if (qok) store_rows_64<T>(reinterpret_cast<E*>(a.out) + (((int64_t)b * N + qi) * a.H + h) * 64, o, g);
    PROF_MARK();
    PROF_FLUSH();
    }   // active
    }   // items
}

}  // namespace

// attn_rpe2d_bwd.hpp — the two-launch backward of attn_rpe2d.hip (every geometry and dtype; the AutoFormer geometry in
// bf16 runs the one-pass kernels of attn_rpe2d_bwd1.hpp / attn_rpe2d_bwd2.hpp unless the batch is too small for them).
//
// With Qx = [Q | X] (X = per-query slot extension of the key-side bucket lookups), Kx = [K | E],
// Vx = [V | E] (E = one-hot slots of the keys), S = scale Qx Kx^T, P = softmax(S),
// [O_pv | SA] = P Vx, O = O_pv + shift(SA) [Tvv; Tvh]:
//     dOx = [dO | gather(dO [Tvv;Tvh]^T)]       dP = dOx Vx^T        delta_i = dO_i . O_i
//     dS = scale P o (dP - delta)               dQx = dS Kx          dK = dS^T Q     dV = P^T dO
//     dQ = dQx[:, :64] + shift(dQx[:, 64:]) [Tkv; Tkh]
//     d[Tkv;Tkh] = shift(dQx[:, 64:])^T Q       d[Tvv;Tvh] = shift(SA)^T dO
// Two launches, both one workgroup per (b,h), no atomics, fixed summation order:
//   A  wave = query tile (lanes own queries): dQ, and the side buffers the second launch needs
//      (slot extensions of Q and dO, delta, the shifted bucket gradients dL'^T)
//   B  wave = key tile (lanes own keys): dK, dV (contraction over queries, so Q^T and dO^T
//      live in LDS), then the four table gradients of this (b,h) as eight 32x32 MFMA jobs.
#pragma once
#include "attn_rpe2d_tile.hpp"

namespace {

// LDS of the dQ kernel: 2 x [K tile | V tile | K^T tile] | key tables^T | table rows (bf16) | masks | scratch
template <typename T> size_t bwd_q_lds_bytes(int NP, int waves, bool fast) {
    using E = typename Tr<T>::elem;
    return 2 * (2 * rm_tile_bytes<T>(64) + t_tile_bytes<T>()) + (size_t)(64 + tabr_rows<T>(4)) * table_pitch<T>() * sizeof(E) +
           (size_t)NP * 4 + (size_t)waves * 32 * LP * 4 + (fast ? onehot_bytes(NP) : 0);
}

template <typename T, bool FAST, bool DROP = false>
__global__ __launch_bounds__(512) void attn_rpe2d_bwd_q_kernel(const BwdArgs a) {
    using TT = Tr<T>;
    using E = typename TT::elem;
    using F = typename TT::frag;
    constexpr int KI = TT::KI, EPL = TT::EPL, S64 = 64 / KI, S32 = 32 / KI;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    static_assert(!FAST || sizeof(E) == 2, "fast path: bf16");
    const RelGeom G = FAST ? RelGeom{197, G14, G14, G14} : a.G;
    const int N = G.n, NP = FAST ? 224 : a.NP;
    const int nt = NP >> 5;
    constexpr int tp = table_pitch<T>(), rp = rm_pitch<T>(64), ktp = t_pitch<T>();
    constexpr size_t set_b = 2 * rm_tile_bytes<T>(64) + t_tile_bytes<T>();
    // stage set i: K rows [32][rp] | V rows [32][rp] | K^T [64][ktp]
    auto kbuf = [&](int i) { return reinterpret_cast<E*>(smem + i * set_b); };
    auto vbuf = [&](int i) { return reinterpret_cast<E*>(smem + i * set_b + rm_tile_bytes<T>(64)); };
    auto ktbuf = [&](int i) { return reinterpret_cast<E*>(smem + i * set_b + 2 * rm_tile_bytes<T>(64)); };
    E* tkt = reinterpret_cast<E*>(smem + 2 * set_b);                      // key tables^T [64][tp]
    E* tkr = tkt + 64 * tp;                                               // key table rows, then value table rows (bf16)
    E* tvr = tkr + tabr_rows<T>(2) * tp;
    uint32_t* masks = reinterpret_cast<uint32_t*>(tkr + tabr_rows<T>(4) * tp);
    float* scratch = reinterpret_cast<float*>(masks + NP);
    short* ohr = reinterpret_cast<short*>(scratch + nt * 32 * LP);   // fast path: one-hot operands (scratch: one slab per query tile)
    short* oht = ohr + NP * OHP;
    const int otp = oht_pitch(NP);

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, g = lane >> 5, c32 = lane & 31;
    const bool active = wave < nt;
    const int qi = wave * 32 + c32;
    const bool qok = qi < N;
    const int qcl = min(qi, N - 1);
    const int qr = qi > 0 ? (qi - 1) / G.gw : 0, qc = qi > 0 ? (qi - 1) - qr * G.gw : 0;
    const int grp = wave >> 2, gt = threadIdx.x & 255;
    // ---- once per (persistent) workgroup: tables, key slot masks, one-hot operands ----------------------------
    {
        TabRegs rk, rv;
        tab_load(rk, a.tkv, a.tkh, a.ldt, a.nb);
        if constexpr (tables_in_lds<T>()) tab_load(rv, a.tvv, a.tvh, a.ldt, a.nb);
        tab_store_T<T>(rk, tkt);
        if constexpr (tables_in_lds<T>()) {
            tab_store_R<T>(rk, tkr);
            tab_store_R<T>(rv, tvr);
        }
    }
    for (int j = threadIdx.x; j < NP; j += blockDim.x) masks[j] = key_mask(j, G);
    if constexpr (FAST) {
        __syncthreads();
        fill_onehot(ohr, oht, masks, NP);
    }
    for (int item = blockIdx.x; item < a.nitems; item += gridDim.x) {
    __syncthreads();                                  // previous item done with the staged tiles / setup published
    const int b = item / a.H, h = item - b * a.H;
    const int64_t bh = (int64_t)b * a.H + h;
    const int64_t base = (int64_t)b * a.sb + (int64_t)h * a.sh;
    const E* qp = reinterpret_cast<const E*>(a.q) + base;
    const E* kpg = reinterpret_cast<const E*>(a.k) + base;
    const E* vpg = reinterpret_cast<const E*>(a.v) + base;
    const int64_t orow = (int64_t)a.H * 64;                               // token stride of out / dout
    const E* dop = reinterpret_cast<const E*>(a.dout) + ((int64_t)b * N * a.H + h) * 64;
    const E* outp = reinterpret_cast<const E*>(a.out) + ((int64_t)b * N * a.H + h) * 64;

    PROF_DECL
    PROF_MARK();
    F qb[S64], dob[S64];
    float delta = 0.f;
    TileRegs<T, 32, 64> sk;
    {
        F ob[S64];
        load_row<T>(qb, qp + (int64_t)qcl * a.sn, g);
        load_row<T>(dob, dop + (int64_t)qcl * orow, g);
        load_row<T>(ob, outp + (int64_t)qcl * orow, g);
        // the workgroup always has 8 waves: waves 0-3 stage the K tiles (rows + transpose), waves
        // 4-7 the V tiles — one chunk per thread, wave-uniform roles (waves >= nt only stage)
        if (grp == 0) tile_load_g<T, 32, 64>(sk, kpg, a.sn, 0, N, 0, gt);
        else tile_load_g<T, 32, 64>(sk, vpg, a.sn, 0, N, 0, gt);


        // delta_i = dO_i . O_i  (this lane holds half of the 64 d-values; the partner the rest)
        if (!qok) { zero_frags<T, S64>(qb); zero_frags<T, S64>(dob); }
#pragma unroll
        for (int ks = 0; ks < S64; ++ks) {
            if constexpr (EPL == 1) delta += dob[ks] * ob[ks];
            else {
#pragma unroll
                for (int e = 0; e < EPL; ++e) delta += TT::to_f(dob[ks][e]) * TT::to_f(ob[ks][e]);
            }
        }
        delta += __shfl_xor(delta, 32);
    }
    if (active && g == 0) a.delta[bh * NP + qi] = delta;
    if (grp == 0) tile_store_g<T, 32, 64, true, sizeof(E) != 2>(sk, kbuf(0), rp, ktbuf(0), ktp, gt);      // bf16: K^T is read with tr16
    else tile_store_g<T, 32, 64, true, false>(sk, vbuf(0), rp, nullptr, 0, gt);
    __syncthreads();                                  // tables, masks, first tiles in place
    PROF_MARK();

    float* scr = scratch + wave * 32 * LP;
    F qe[S32], de[S32];
    if (active) {
        table_lookups<T>(scr, qb, tkr, a.tkv, a.tkh, a.ldt, a.nb, lane);
        wave_lds_fence();
        if constexpr (FAST) build_ext14(qe, scr, lane, wave == 0, qr, qc);
        else build_ext<T>(qe, scr, lane, qi, qr, qc, G);
        wave_lds_fence();
        table_lookups<T>(scr, dob, tvr, a.tvv, a.tvh, a.ldt, a.nb, lane);
        wave_lds_fence();
        if constexpr (FAST) build_ext14(de, scr, lane, wave == 0, qr, qc);
        else build_ext<T>(de, scr, lane, qi, qr, qc, G);
        wave_lds_fence();
        store_ext_rows<T>(reinterpret_cast<E*>(a.qe) + (bh * NP + qi) * 32, qe, g);
        store_ext_rows<T>(reinterpret_cast<E*>(a.de) + (bh * NP + qi) * 32, de, g);
    }
    PROF_MARK();

    const float sc = a.scale * LOG2E;
    const float m2 = (active && qok) ? a.lse[bh * N + qi] * LOG2E : 0.f;

    f32x16 dq[2] = {f32x16{}, f32x16{}};
    f32x16 dx = {};
    for (int t = 0; t < nt; ++t) {
        const int cur = t & 1;
        if (t + 1 < nt) {
            if (grp == 0) tile_load_g<T, 32, 64>(sk, kpg, a.sn, (t + 1) * 32, N, 0, gt);
            else tile_load_g<T, 32, 64>(sk, vpg, a.sn, (t + 1) * 32, N, 0, gt);
        }
        if (active) {
            const E* kb = kbuf(cur) + c32 * rp;
            const E* vb = vbuf(cur) + c32 * rp;
            f32x16 sacc = {}, pacc = {};
#pragma unroll
            for (int ks = 0; ks < S64; ++ks) {
                sacc = TT::mma(TT::load(kb + ks * KI + g * EPL), qb[ks], sacc);
                pacc = TT::mma(TT::load(vb + ks * KI + g * EPL), dob[ks], pacc);
            }
            uint32_t km = 0;
            if constexpr (!FAST) km = masks[t * 32 + c32];
#pragma unroll
            for (int ks = 0; ks < S32; ++ks) {
                F oh;
                if constexpr (FAST) oh = TT::load(ohr + (t * 32 + c32) * OHP + ks * KI + g * EPL);
                else oh = TT::onehot_row(km, ks, g);
                sacc = TT::mma(oh, qe[ks], sacc);
                pacc = TT::mma(oh, de[ks], pacc);
            }
            // dS^T = scale * P o (dP - delta), keys beyond N contribute nothing
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const bool ok = t * 32 + acc_row(r, g) < N;
                const float p = ok ? __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[r], sc, -m2)) : 0.f;
                if constexpr (DROP)                   // dP = keep / (1 - p) o (dO Vx^T): the mask sits on dP, P stays undropped
                    pacc[r] = drop_keep(drop_key(a.drop_seed, item), qi, t * 32 + acc_row(r, g), a.drop_thr) ? pacc[r] * a.drop_scale : 0.f;
                sacc[r] = p * (pacc[r] - delta) * a.scale;
            }
            const E* ktb = ktbuf(cur);
#pragma unroll
            for (int st = 0; st < S32; ++st) {
                const F db = TT::from_acc(sacc, st);
                dq[0] = TT::mma(perm_operand<T>(kbuf(cur), rp, ktb, ktp, 0, st, lane), db, dq[0]);
                dq[1] = TT::mma(perm_operand<T>(kbuf(cur), rp, ktb, ktp, 1, st, lane), db, dq[1]);
                if constexpr (FAST) dx = TT::mma(TT::load_perm(oht + c32 * otp + t * 32, st, g), db, dx);
                else dx = TT::mma(TT::onehot_perm(masks + t * 32, st, g, c32), db, dx);
            }
        }
        if (t + 1 < nt) {
            if (grp == 0) tile_store_g<T, 32, 64, true, sizeof(E) != 2>(sk, kbuf(cur ^ 1), rp, ktbuf(cur ^ 1), ktp, gt);
            else tile_store_g<T, 32, 64, true, false>(sk, vbuf(cur ^ 1), rp, nullptr, 0, gt);
            __syncthreads();
        }
    }
    PROF_MARK();
    if (active) {

    float bk[32];
    if constexpr (FAST) slots_to_buckets14(bk, scr, dx, lane, wave == 0, min(qr, G14 - 1), qc);
    else slots_to_buckets(bk, scr, dx, lane, qi, qr, qc, G);
    // dL'^T (64 buckets x NP queries) for the table gradients of launch B
    store_buckets_T<T>(reinterpret_cast<E*>(a.dlt) + bh * 64 * NP + qi, NP, bk, g);
    add_bucket_product<T>(dq, tkt, bk, lane);
    if (qok)
        store_rows_64<T>(reinterpret_cast<E*>(a.dq) + (int64_t)b * a.dsb + (int64_t)qi * a.dsn + (int64_t)h * a.dsh,
                         dq, g);
    PROF_MARK();
    PROF_FLUSH();
    }   // active
    }   // items
}

// LDS of the dK/dV kernel: 2 x [Q | dO rows, Q^T | dO^T, qe | de rows, dL'^T | S'^T tiles] | lse2 | delta
template <typename T> __host__ __device__ constexpr size_t kv_set_bytes() {
    return 2 * rm_tile_bytes<T>(64) + 2 * t_tile_bytes<T>() + 2 * rm_tile_bytes<T>(32) + 2 * t_tile_bytes<T>();
}
template <typename T> size_t bwd_kv_lds_bytes(int NP) { return 2 * kv_set_bytes<T>() + (size_t)NP * 8; }

template <typename T, bool DROP = false>
__global__ __launch_bounds__(512) void attn_rpe2d_bwd_kv_kernel(const BwdArgs a) {
    using TT = Tr<T>;
    using E = typename TT::elem;
    using F = typename TT::frag;
    constexpr int KI = TT::KI, EPL = TT::EPL, S64 = 64 / KI, S32 = 32 / KI;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const RelGeom G = a.G;
    const int N = G.n, NP = a.NP;
    const int nt = NP >> 5;
    constexpr int rp = rm_pitch<T>(64), ep = rm_pitch<T>(32), tpt = t_pitch<T>();
    constexpr size_t RB = rm_tile_bytes<T>(64), TB = t_tile_bytes<T>(), EB = rm_tile_bytes<T>(32), SET = kv_set_bytes<T>();
    // stage set i: Q rows | dO rows | Q^T | dO^T | qe rows | de rows | dL'^T tile [64 u][tpt] | S'^T tile
    auto qbuf = [&](int i) { return reinterpret_cast<E*>(smem + i * SET); };
    auto dbuf = [&](int i) { return reinterpret_cast<E*>(smem + i * SET + RB); };
    auto qtbuf = [&](int i) { return reinterpret_cast<E*>(smem + i * SET + 2 * RB); };
    auto dtbuf = [&](int i) { return reinterpret_cast<E*>(smem + i * SET + 2 * RB + TB); };
    auto qebuf = [&](int i) { return reinterpret_cast<E*>(smem + i * SET + 2 * RB + 2 * TB); };
    auto debuf = [&](int i) { return reinterpret_cast<E*>(smem + i * SET + 2 * RB + 2 * TB + EB); };
    auto dlbuf = [&](int i) { return reinterpret_cast<E*>(smem + i * SET + 2 * RB + 2 * TB + 2 * EB); };
    auto spbuf = [&](int i) { return reinterpret_cast<E*>(smem + i * SET + 2 * RB + 3 * TB + 2 * EB); };
    float* lse2 = reinterpret_cast<float*>(smem + 2 * SET);               // [NP]
    float* dlt_s = lse2 + NP;                                             // delta [NP]

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nwaves = blockDim.x >> 6;
    const int lane = threadIdx.x & 63, g = lane >> 5, c32 = lane & 31;
    // persistent workgroup: (b, h) items blockIdx.x, + gridDim.x, ...  The item-specific operands of the NEXT item (own
    // K / V rows, first staged tile set, lse / delta) are requested into registers before the current item's epilogue
    // (dK / dV and table-gradient stores), so an item starts with its prologue loads already landed: the prologue was
    // 21 % of an item (phase stamps of tools/probes/attn_probe).
    struct ItemPtrs {
        const E *qp, *kpg, *vpg, *dop, *qep, *dep, *dltp, *spp;
        int64_t bh;
        int b, h;
    };
    const int64_t orow = (int64_t)a.H * 64;
    auto item_ptrs = [&](int item) {
        ItemPtrs P;
        P.b = item / a.H;
        P.h = item - P.b * a.H;
        P.bh = (int64_t)P.b * a.H + P.h;
        const int64_t base = (int64_t)P.b * a.sb + (int64_t)P.h * a.sh;
        P.qp = reinterpret_cast<const E*>(a.q) + base;
        P.kpg = reinterpret_cast<const E*>(a.k) + base;
        P.vpg = reinterpret_cast<const E*>(a.v) + base;
        P.dop = reinterpret_cast<const E*>(a.dout) + ((int64_t)P.b * N * a.H + P.h) * 64;
        P.qep = reinterpret_cast<const E*>(a.qe) + P.bh * NP * 32;
        P.dep = reinterpret_cast<const E*>(a.de) + P.bh * NP * 32;
        P.dltp = reinterpret_cast<const E*>(a.dlt) + P.bh * 64 * NP;
        P.spp = reinterpret_cast<const E*>(a.sp) + P.bh * 64 * NP;
        return P;
    };
    const bool active = wave < nt;
    const int kj = wave * 32 + c32;
    const bool kok = active && kj < N;

    // staging is split over two groups of four waves (the workgroup always has 8 waves; waves
    // >= nt only stage): group 0 moves the Q tile (+ its transpose), the qe | de rows and the S'^T
    // tile, group 1 the dO tile (+ transpose) and the dL'^T tile — wave-uniform roles, every
    // thread of a group has exactly one chunk per tile
    const int grp = wave >> 2, gt = threadIdx.x & 255;
    TileRegs<T, 32, 64> sq;                                  // group 0: Q rows      group 1: dO rows
    TileRegs<T, 64, 32> sdl;                                 // group 0: S'^T tile   group 1: dL'^T tile
    constexpr int EH = TileRegs<T, 32, 32>::CH;              // chunks of one 32 x 32 extension tile
    TileRegs<T, 32, 32> sqe;                                 // group 0 only: qe (first half of the group) | de
    auto load_set = [&](const ItemPtrs& P, int t) {
        if (grp == 0) {
            tile_load_g<T, 32, 64>(sq, P.qp, a.sn, t * 32, N, 0, gt);
            tile_load_g<T, 64, 32>(sdl, P.spp, NP, 0, 64, t * 32, gt);
            if constexpr (EH == 128) {                       // bf16: 128 chunks each -> half a group per tile
                const int c = gt & 127, row = c >> 2, cc = c & 3;
                const E* src = (gt < 128 ? P.qep : P.dep) + (int64_t)(t * 32 + row) * 32 + cc * 8;
                sqe.v[0] = *reinterpret_cast<const u32x4v*>(src);
            } else {                                         // fp32: 256 chunks each -> two per thread
                tile_load_g<T, 32, 32>(sqe, P.qep, 32, t * 32, NP, 0, gt);
            }
        } else {
            tile_load_g<T, 32, 64>(sq, P.dop, orow, t * 32, N, 0, gt);
            tile_load_g<T, 64, 32>(sdl, P.dltp, NP, 0, 64, t * 32, gt);
        }
    };
    TileRegs<T, 32, 32> sde;                                 // fp32 only: de rows (group 0)
    auto load_set_extra = [&](const ItemPtrs& P, int t) {
        if constexpr (EH != 128) { if (grp == 0) tile_load_g<T, 32, 32>(sde, P.dep, 32, t * 32, NP, 0, gt); }
    };
    auto store_set = [&](int i) {
        if (grp == 0) {
            tile_store_g<T, 32, 64, true, sizeof(E) != 2>(sq, qbuf(i), rp, qtbuf(i), tpt, gt);     // bf16: Q^T / dO^T are read with tr16
            tile_store_g<T, 64, 32, true, false>(sdl, spbuf(i), tpt, nullptr, 0, gt);
            if constexpr (EH == 128) {
                const int c = gt & 127, row = c >> 2, cc = c & 3;
                E* d = (gt < 128 ? qebuf(i) : debuf(i)) + row * ep + cc * 8;
                *reinterpret_cast<u32x4v*>(d) = sqe.v[0];
            } else {
                tile_store_g<T, 32, 32, true, false>(sqe, qebuf(i), ep, nullptr, 0, gt);
                tile_store_g<T, 32, 32, true, false>(sde, debuf(i), ep, nullptr, 0, gt);
            }
        } else {
            tile_store_g<T, 32, 64, true, sizeof(E) != 2>(sq, dbuf(i), rp, dtbuf(i), tpt, gt);
            tile_store_g<T, 64, 32, true, false>(sdl, dlbuf(i), tpt, nullptr, 0, gt);
        }
    };
    // the one-hot slot operand of this lane's key: geometry only
    F oh[S32];
    {
        const uint32_t km = key_mask(kj, G);
#pragma unroll
        for (int ks = 0; ks < S32; ++ks) oh[ks] = TT::onehot_row(km, ks, g);
    }
    const float sc = a.scale * LOG2E;

    // requests of an item's prologue operands (NP <= 256 < blockDim: one lse / delta value per thread)
    F kb[S64], vb[S64];
    float lse_r = INFINITY, dlt_r = 0.f;
    auto request_item = [&](const ItemPtrs& P) {
        load_row<T>(kb, P.kpg + (int64_t)min(kj, N - 1) * a.sn, g);
        load_row<T>(vb, P.vpg + (int64_t)min(kj, N - 1) * a.sn, g);
        load_set(P, 0);
        load_set_extra(P, 0);
        const int i = threadIdx.x;
        lse_r = i < N ? a.lse[P.bh * N + i] * LOG2E : INFINITY;           // P = 0 for padding queries
        dlt_r = i < N ? a.delta[P.bh * NP + i] * a.scale : 0.f;
    };
    // table-gradient jobs of this wave: job = tab*2 + dt (tab 0/1 key tables v/h: X = Q, R = dL';
    // tab 2/3 value tables: X = dO, R = S'), dT^T(64 d x 32 u) = X^T(d x q) . R(q x u).  The tables are shared by all
    // (b, h): the accumulators live across the workgroup's items and ONE partial per workgroup leaves the kernel
    // (256 x 32 KB instead of B*H x 32 KB written here and read back by the gradient finalisation).
    const int job0 = wave, job1 = wave + nwaves;      // nwaves >= 4 -> at most two jobs per wave
    f32x16 tacc[2] = {f32x16{}, f32x16{}};

    int item = blockIdx.x;
    if (item >= a.nitems) return;
    ItemPtrs P = item_ptrs(item);
    request_item(P);

    for (;;) {
    __syncthreads();                                  // previous item done with the staged tiles and lse / delta
    const int b = P.b, h = P.h;
    [[maybe_unused]] const int64_t bh = P.bh;
    PROF_DECL
    PROF_MARK();
    if (threadIdx.x < NP) { lse2[threadIdx.x] = lse_r; dlt_s[threadIdx.x] = dlt_r; }
    store_set(0);
    __syncthreads();
    PROF_MARK();


    f32x16 dk[2] = {f32x16{}, f32x16{}}, dv[2] = {f32x16{}, f32x16{}};
    for (int t = 0; t < nt; ++t) {
        const int cur = t & 1;
        PROF_LOOP(t);
        if (t + 1 < nt) { load_set(P, t + 1); load_set_extra(P, t + 1); }
        if (active) {
            const E* qrow = qbuf(cur) + c32 * rp;
            const E* drow = dbuf(cur) + c32 * rp;
            const E* qerow = qebuf(cur) + c32 * ep;
            const E* derow = debuf(cur) + c32 * ep;
            f32x16 sacc = {}, pacc = {};
#pragma unroll
            for (int ks = 0; ks < S64; ++ks) {
                sacc = TT::mma(TT::load(qrow + ks * KI + g * EPL), kb[ks], sacc);
                pacc = TT::mma(TT::load(drow + ks * KI + g * EPL), vb[ks], pacc);
            }
#pragma unroll
            for (int ks = 0; ks < S32; ++ks) {
                sacc = TT::mma(TT::load(qerow + ks * KI + g * EPL), oh[ks], sacc);
                pacc = TT::mma(TT::load(derow + ks * KI + g * EPL), oh[ks], pacc);
            }
            PROF_LOOP(t);
            // lane = key, registers = queries t*32 + acc_row(r, g) — four runs of four consecutive
            // queries, so lse / delta come as 16-byte LDS reads; padding queries have lse2 = +inf
            // (P = 0).  Padding KEYS (lanes kj >= N) need no masking: a key is a COLUMN of every
            // product below, its values never mix into other lanes, and its rows are not stored.
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                const f32x4v l4 = *reinterpret_cast<const f32x4v*>(lse2 + t * 32 + 8 * r4 + 4 * g);
                const f32x4v d4 = *reinterpret_cast<const f32x4v*>(dlt_s + t * 32 + 8 * r4 + 4 * g);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = 4 * r4 + e;
                    const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[r], sc, -l4[e]));
                    if constexpr (DROP) {                                         // dV takes the dropped map, dS the mask on dP
                        const bool keep = drop_keep(drop_key(a.drop_seed, item), t * 32 + 8 * r4 + 4 * g + e, kj, a.drop_thr);
                        sacc[r] = keep ? p * a.drop_scale : 0.f;
                        pacc[r] = p * __builtin_fmaf(keep ? pacc[r] * a.drop_scale : 0.f, a.scale, -d4[e]);
                    } else {
                    sacc[r] = p;
                    pacc[r] = p * __builtin_fmaf(pacc[r], a.scale, -d4[e]);      // dlt_s holds scale * delta
                    }
                }
            }
            PROF_LOOP(t);
#pragma unroll
            for (int st = 0; st < S32; ++st) {
                const F pb = TT::from_acc(sacc, st);
                const F db = TT::from_acc(pacc, st);
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    dv[dt] = TT::mma(perm_operand<T>(dbuf(cur), rp, dtbuf(cur), tpt, dt, st, lane), pb, dv[dt]);
                    dk[dt] = TT::mma(perm_operand<T>(qbuf(cur), rp, qtbuf(cur), tpt, dt, st, lane), db, dk[dt]);
                }
            }
        }
        PROF_LOOP(t);
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int job = jj == 0 ? job0 : job1;
            if (job < 8) {
                const int tab = job >> 1, dt = job & 1;
                const E* xR = tab < 2 ? qbuf(cur) : dbuf(cur);
                const E* xT = tab < 2 ? qtbuf(cur) : dtbuf(cur);
                const E* rT = (tab < 2 ? dlbuf(cur) : spbuf(cur)) + ((tab & 1) * 32 + c32) * tpt;
#pragma unroll
                for (int st = 0; st < S32; ++st)
                    tacc[jj] = TT::mma(perm_operand<T>(xR, rp, xT, tpt, dt, st, lane), TT::load_perm(rT, st, g), tacc[jj]);
            }
        }
        PROF_LOOP(t);
        if (t + 1 < nt) {
            store_set(cur ^ 1);
            PROF_LOOP(t);
            __syncthreads();
        }
        PROF_LOOP(t);
    }
    PROF_MARK();
    // the next item's prologue operands travel while this item's results are stored
    const int next = item + gridDim.x;
    const bool more = next < a.nitems;
    if (more) {
        P = item_ptrs(next);
        request_item(P);
    }
    if (kok) {
        const int64_t off = (int64_t)b * a.dsb + (int64_t)kj * a.dsn + (int64_t)h * a.dsh;
        store_rows_64<T>(reinterpret_cast<E*>(a.dk) + off, dk, g);
        store_rows_64<T>(reinterpret_cast<E*>(a.dv) + off, dv, g);
    }
    PROF_MARK();
    PROF_MARK();
    PROF_FLUSH();
    if (!more) break;
    item = next;
    }   // items
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
        const int job = jj == 0 ? job0 : job1;
        if (job < 8) {
            // lane = bucket u (column), registers = d rows
            const int tab = job >> 1, dt = job & 1;
            float* dst = a.dtab + (((int64_t)blockIdx.x * 4 + tab) * 32 + c32) * 64 + dt * 32;
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4)
                *reinterpret_cast<f32x4v*>(dst + 8 * r4 + 4 * g) =
                    f32x4v{tacc[jj][4 * r4], tacc[jj][4 * r4 + 1], tacc[jj][4 * r4 + 2], tacc[jj][4 * r4 + 3]};
        }
    }
}

}  // namespace
